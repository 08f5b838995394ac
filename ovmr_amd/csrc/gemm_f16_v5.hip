// fp16 MFMA GEMM, the tile kernel of variants 6 and 8 (the default): 256(128)x256x64 tiles, both operands streamed into LDS by LDS-DMA
// (global_load_lds, 16 B per lane, XOR-swizzled 128-byte rows), 8 waves as 2 x 4.  K loops: the ping-pong loop (four half-tiles per
// K-tile, counted vmcnt, the two wave rows one barrier apart: see OPT_PINGPONG below; r02: qkv 369 -> 312, c_fc 522 -> 461,
// c_proj 462 -> 387, out_proj 149 -> 132 us at batch 512); the double buffer with a drain per K-tile and software-pipelined fragment
// reads; and that with the iteration boundary moved inside the MFMA stream (OPT_BOUNDARY).  Tile height, K loop and cache hints of a
// launch are gemm_f16_route's decision (gemm_f16.hip, with the measurements behind each rule); the table at the end of this file holds
// the instantiations it can ask for.
//
// Epilogue (measured with tools/gemm_bench.py variants 6 / 18 / 19, profiles/r01g_gemm_epilogue.md: with K = 768 the
// epilogue was 24-44 % of the kernel, the K loop alone runs at 1.1-1.2 PFLOP/s):
//   * EVERYTHING THE EPILOGUE READS IS STAGED IN LDS AT KERNEL START -- bias (or the LayerNorm-fold column constants) of the
//     tile's 256 columns and, for the LN-folding epilogues, rstd / -rstd*mean of its rows.  Their global-load latency hides
//     under the first K-tile's; loading them after the K loop put ~1-2 us of exposed latency in front of every tile's stores;
//   * results go THROUGH LDS: the C^T accumulator layout gives each lane 4 consecutive columns of 32 (row, column-tile)
//     pairs; h(acc + bias) (+QuickGELU / scale / LN fold) is written to a per-wave LDS tile and read back row-major, so
//     residual / positional rows are LOADED and results STORED 16 bytes per lane, 8 rows x 128 B per wave instruction;
//   * residual rows (EPI_BIAS_RES) are requested before the accumulators are converted, not in front of each store;
//   * large outputs are stored with the NONTEMPORAL hint (OPT_NT_STORE): C then stops evicting the A / W panels the
//     other tiles of the XCD are streaming out of its 4 MiB L2 (qkv 404 -> 368 us, c_fc 587 -> 556 us);
//   * EPI_BIAS_RES can emit per-row partial (sum, sum of squares) for the LayerNorm that follows (common.h);
//   * ONE workgroup barrier in the epilogue (the staging tiles are wave-private; the barriers that used to separate the
//     phases also drained the first half's global stores), packed fp32 / fp16 VALU forms, interior tiles without bounds
//     compares.
// Tile loop (the LayerNorm-folding ping-pong instantiations, v5_tile_loop: in_proj <6, 8, 528> and c_fc <7, 8, 2576>; r07a, DESIGN.md
// section 4).  A workgroup walks the dispatch slots blockIdx.x, + gridDim.x, ...; a slot is a tile by the same XCD-aware map as a
// block id (v5_tile_of), so a CU computes the tiles it was dispatched before, in the same order.  Where the route plans it
// (GemmPlan::persist) the grid is one workgroup per CU; with one workgroup per tile the loop runs once.  A one-tile workgroup ends
// behind its last global_store, the hardware holds it until every store is acknowledged, and only then the CU's next workgroup is
// dispatched and pays the operand latency of its prologue: acknowledgement, dispatch and first-tile latency one after the other,
// per tile and CU.  In the loop:
//   * LDS is 2 x 64 KiB of K slots, TWO 4 KiB constant blocks (tile t uses block t & 1) and 16 KiB of epilogue staging, 2 KiB per
//     wave: results go through LDS in steps of 16 accumulator rows instead of two 64-row halves laid over the K slots, so that the
//     K slots belong to the next tile as soon as the K loop is over.  What was traded: a step needs the constants of all four column
//     blocks, so the 2 x 16 column constants of a lane are held in registers for the whole epilogue, and the conversions of a step
//     are kept behind the step before (sched_barrier) -- 256 VGPRs, no scratch (234 before);
//   * behind the K loop's last barrier (the balancing one: every wave of both rows has retired its last fragment read in front of
//     the barrier it arrives at, so every K slot is free -- the WAR rule of the K loop) the workgroup issues the NEXT tile's prologue
//     DMA -- K-tile 0 and the first two half-tiles of K-tile 1, the prologue's six stage_half -- and, in front of them, plain loads
//     of the next tile's column constants and row statistics into registers; only then it converts and stores this tile, and last
//     it computes rstd / -rstd * mean from those registers and writes the other constant block;
//   * which wait retires what.  The next tile's K-tile 0: the loop top's counted vmcnt(4) + lgkmcnt(0) + s_barrier, the same three
//     instructions as the prologue's.  The counter counts this tile's 16 stores too, which were issued AFTER the twelve DMAs: "at
//     most 4 outstanding" leaves, among the loads, at most the newest four = the two half-tiles of K-tile 1 (loads retire in order
//     among themselves; no order between loads and stores is assumed), so K-tile 0 has landed whatever the stores do, and every
//     later counted wait of the K loop is only the stronger for stores still in flight.  The wait therefore costs the later of
//     {operand latency, store acknowledgement}, both started a whole epilogue earlier, and no dispatch.  There is no
//     __syncthreads() and no vmcnt(0) between a tile's last store and the next tile's first MFMA;
//   * the constant loads are hipcc's own: it waits for them in front of the arithmetic at the END of the epilogue, counting that
//     epilogue's 16 stores -- vmcnt(16) on interior tiles, which drains none of them (the interior and the guarded form each end
//     with their own copy of that code for this reason).  A guarded tile (last row / column of tiles), whose store count is not
//     known, gets vmcnt(0) there, and so does a launch with more than four statistics slots (K > 1024: the slots beyond four are
//     read at that point);
//   * the constant block written at the end of tile t is first read after the K loop of tile t + 1 (barriers in between), and was
//     last read in the epilogue of tile t - 1; the staging area is private to its wave (LDS executes a wave's instructions in order).
// tests/test_hip_gemm_persist.py drives the loop on shapes of a few tiles with the grid capped (ovmr_debug_gemm_persist).
// Measured and removed (profiles/r01e_gemm_experiments.md, r01g_gemm_epilogue.md): L2 prefetch touches (every workgroup, and
// designated prefetcher workgroups), staggered LDS-DMA issue, buffer_load ... lds, s_setprio around the MFMA stream, a
// persistent one-workgroup-per-CU tile loop with the next tile's first K-tile prefetched under the epilogue, W fragments
// straight from global memory, tile-contiguous C stores, residual as accumulator start value, x ping-pong buffers.
#include <algorithm>
#include <type_traits>

#include "gemm_route.h"

namespace {

constexpr int BK5 = 64, BN5 = 256;
typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}

// OPT bits (the values are part of the kernels' names: bench.py, tests/test_isa_sync_templates.py)
constexpr int OPT_A_NT = 1;           // nontemporal LDS-DMA for the A operand
constexpr int OPT_BOUNDARY = 4;       // K loop with the iteration boundary inside the MFMA stream
constexpr int OPT_PINGPONG = 16;      // the ping-pong K loop (256-row tiles)
constexpr int OPT_NT_STORE = 512;     // nontemporal C stores (a template bit: the compiler merges a run-time branch around two stores of the
                                      // same value and drops the hint)
constexpr int OPT_GELU_F32 = 2048;    // the fp32 QuickGELU form

// The LayerNorm-folding ping-pong instantiations (in_proj, c_fc) are written as a TILE LOOP: a workgroup walks the dispatch slots
// blockIdx.x, + gridDim.x, ... (launched with one workgroup per tile the loop runs once; see the kernel's ping-pong section).
constexpr bool v5_tile_loop(int epi, int mt, int opt) { return (epi == EPI_LN_BIAS || epi == EPI_LN_BIAS_QGELU) && mt == 8 && (opt & OPT_PINGPONG); }
constexpr int V5_CONST_BLOCK = 4096, V5_STAGING = 16384;   // tile loop: two constant blocks and the epilogue's staging behind the K buffers

// dispatch slot (block id) -> tile.  XCD-aware: ids congruent mod 8 run on one XCD and get a contiguous range of tiles; inside the
// range N tiles come in groups of G with M fastest-but-one (n_group, set by gemm_f16_route).
__host__ __device__ __forceinline__ void v5_tile_of(int bid, int tiles_m, int tiles_n, int n_group, int& tm, int& tn) {
    const int nwg = tiles_m * tiles_n;
    {
        const int xcd = bid & 7, idx = bid >> 3, q = nwg >> 3, r = nwg & 7;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int G = n_group > 0 ? n_group : tiles_n;
    const int full = tiles_n / G, per = tiles_m * G;
    const int g = bid / per;
    if (g < full) {
        const int r = bid - g * per;
        tm = r / G;
        tn = g * G + (r - tm * G);
    } else {
        const int Gl = tiles_n - full * G, r = bid - full * per;
        tm = r / Gl;
        tn = full * G + (r - tm * Gl);
    }
}

template <int EPI, int MT, int OPT>
__global__ __launch_bounds__(512) void gemm_f16_v5_kernel(GemmArgs a, int tiles_m, int tiles_n) {
    constexpr int BM = MT * 32;
    constexpr int A_BYTES = BM * 128, STAGE = (BM + BN5) * 128;
    constexpr int AJ = BM / 64;
    constexpr bool NT = OPT & OPT_NT_STORE;
    constexpr int EP = 128;                            // epilogue staging tile: 128-byte rows, swizzled 8-byte units (below)
    constexpr bool GFAST = (OPT & OPT_GELU_F32) != 0;  // QuickGELU: the one-rounding fp32 form (common.h quick_gelu_f32x2) instead of the reference's three fp16 rounding points
    constexpr bool LNF = EPI == EPI_LN_BIAS || EPI == EPI_LN_BIAS_QGELU;   // LayerNorm folded into this GEMM (common.h)
    constexpr bool HAS_BIAS = EPI == EPI_BIAS || EPI == EPI_BIAS_QGELU || EPI == EPI_BIAS_RES;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // behind the two K buffers: column constants [2][256] fp32, row constants [2][BM] fp32
    float* col_c = (float*)(smem + 2 * STAGE);
    float* row_c = col_c + 2 * BN5;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;

    constexpr bool LOOPED = v5_tile_loop(EPI, MT, OPT);   // the tile loop (ping-pong section): m0 / n0 move on to the workgroup's next tile
    int tm, tn;
    v5_tile_of(blockIdx.x, tiles_m, tiles_n, a.n_group, tm, tn);
    int m0 = tm * BM, n0 = tn * BN5;

    const int nk = a.K / BK5;
    const half_t* A = (const half_t*)a.A;
    const half_t* W = (const half_t*)a.W;

    // staging: lane -> (row within the 8-row group, destination slot); source chunk = slot ^ row
    const int srow = lane >> 3, slot = lane & 7;
    const int schunk = (slot ^ srow) * 8;
    unsigned oa[AJ], ob[4];                            // byte offsets of this lane's source rows
    // row-major: row * ld * 2 + chunk, K-tile step 128 B
    auto src_off = [&](int row, int ld) -> unsigned { return (unsigned)(((long)row * ld + schunk) * 2); };
    // EPI_PATCH with a.im2col_R: the A operand is the image tensor [B, 3, R, R] (fp16) and row r = patch (b, gy, gx) of the 16 x 16
    // grid cells.  K-tile kt holds k = kt*64 .. +63 = channel kt >> 2, pixel rows 4 (kt & 3) .. +3 of the patch, 16 pixels each: the
    // 16-byte chunk c8 of a row is pixel row c8 >> 1, pixels 8 (c8 & 1) .. +7.  So a lane's source is (row part + chunk part) + a
    // K-tile part that is the same for every lane -- exactly the scalar-base + lane-offset form of the DMA.
    const int imR = (EPI == EPI_PATCH) ? a.im2col_R : 0;
    auto a_off = [&](int row) -> unsigned {
        if (EPI == EPI_PATCH && imR) {
            const int G = imR >> 4, r = min(row, a.M - 1), b = r / a.rows_in, p = r - b * a.rows_in, gy = p / G, gx = p - gy * G;
            const int c8 = schunk >> 3;
            return (unsigned)(2 * (((long)b * 3 * imR + gy * 16 + (c8 >> 1)) * imR + gx * 16 + (c8 & 1) * 8));
        }
        return src_off(min(row, a.M - 1), a.lda);
    };
    auto a_tile = [&](int kt) -> const char* {           // wave-uniform
        if (EPI == EPI_PATCH && imR) return (const char*)A + 2 * ((long)(kt >> 2) * imR * imR + (kt & 3) * 4 * imR);
        return (const char*)A + (long)kt * 128;
    };
#pragma unroll
    for (int j = 0; j < AJ; ++j) {
        const int r = m0 + wave * (BM / 8) + j * 8 + srow;
        oa[j] = a_off(r);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = n0 + wave * 32 + j * 8 + srow;
        ob[j] = src_off(min(r, a.N - 1), a.ldw);
    }
    const int ldsA_w = wave * (BM / 8) * 128;
    const int ldsB_w = A_BYTES + wave * 32 * 128;

    auto stage = [&](int buf, int kt) {
        char* base = smem + buf * STAGE;
#pragma unroll
        for (int j = 0; j < AJ; ++j)
            __builtin_amdgcn_global_load_lds((gptr_t)(a_tile(kt) + oa[j]), (lptr_t)(base + ldsA_w + j * 1024), 16, 0, (OPT & OPT_A_NT) ? 2 : 0);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            __builtin_amdgcn_global_load_lds((gptr_t)((const char*)W + ob[j] + (long)kt * 128), (lptr_t)(base + ldsB_w + j * 1024), 16, 0, 0);
    };

    float4_t acc[MT][4];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (float4_t){0.f, 0.f, 0.f, 0.f};

    const int fr = lane & 15, fg = lane >> 4;
    const int a_row_off = (wm * (BM / 2) + fr) * 128;
    const int b_row_off = A_BYTES + (wn * 64 + fr) * 128;
    const int ch0 = ((fg) ^ (fr & 7)) << 4, ch1 = ((4 + fg) ^ (fr & 7)) << 4;

    // LayerNorm fold of one accumulator block's four columns (both epilogues below): rstd * acc + (c1 - rstd * mean * c0), QuickGELU, fp16
    auto ln_fold4 = [&](const float4_t v, const float ln_r, const float ln_t, const float4_t c0, const float4_t c1) -> half4_t {
        half4_t o;
#pragma unroll
        for (int r = 0; r < 4; r += 2) {
            // two columns per instruction (v_pk_fma_f32): same two fused multiply-adds per element as the scalar form
            const float2_t t2 = __builtin_elementwise_fma((float2_t){ln_t, ln_t}, (float2_t){c0[r], c0[r + 1]}, (float2_t){c1[r], c1[r + 1]});
            float2_t x2 = __builtin_elementwise_fma((float2_t){ln_r, ln_r}, (float2_t){v[r], v[r + 1]}, t2);
            if (EPI == EPI_LN_BIAS_QGELU && GFAST) x2 = quick_gelu_f32x2(x2);
            const half2_t u2 = __builtin_convertvector(x2, half2_t);
            o[r] = u2[0];
            o[r + 1] = u2[1];
        }
        if (EPI == EPI_LN_BIAS_QGELU && !GFAST) o = quick_gelu_h4(o);
        return o;
    };
    // epilogue staging tile (both epilogues; the swizzle is described at the epilogue below): byte offset at which a lane writes column
    // block j of its row fr, byte offset of the 16-byte chunk it reads back from row lane >> 3, and the halves of a chunk put back
    auto stage_wr = [&](int j) -> int { return fr * EP + (((j * 4 + fg) ^ (((fr & 7) << 1) | (fr >> 3))) << 3); };
    auto stage_rd = [&]() -> int { return (lane >> 3) * EP + (((lane & 7) ^ (lane >> 3)) << 4); };
    auto stage_unswap = [](const half8_t v, int it) -> half8_t {
        if (it & 1) return (half8_t){v[4], v[5], v[6], v[7], v[0], v[1], v[2], v[3]};
        return v;
    };

    constexpr bool PH8 = (OPT & OPT_PINGPONG) != 0 && MT == 8;
    if (!PH8) stage(0, 0);

    // epilogue constants -> LDS, under the latency of the first K-tile (first read after the K loop: many barriers later).  (The same
    // block stands in the ping-pong prologue below: as one lambda called at both points it changed the register allocation and the
    // schedule of every kernel with a bias or a LayerNorm fold.)
    if (PH8) {
    } else if (tid < BN5) {
        const int n = n0 + tid;
        float c0 = 0.f, c1 = 0.f;
        if (n < a.N) {
            if (HAS_BIAS) c0 = (float)((const half_t*)a.bias)[n];
            if (LNF) { c0 = a.ln_g[n]; c1 = a.ln_b[n]; }
        }
        col_c[tid] = c0;
        col_c[BN5 + tid] = c1;
    } else if (LNF && tid - BN5 < BM) {
        const int r = tid - BN5;
        const float2_t* sp = (const float2_t*)a.ln_stats + (long)min(m0 + r, a.M - 1) * (a.ln_stride ? a.ln_stride : a.ln_slots);
        float su = 0.f, sq = 0.f;
        for (int sl = 0; sl < a.ln_slots; ++sl) { const float2_t p = sp[sl]; su += p[0]; sq += p[1]; }
        const float inv_k = 1.0f / (float)a.K;
        const float mean = su * inv_k;
        const float rstd = 1.0f / sqrtf(fmaxf(sq * inv_k - mean * mean, 0.f) + 1e-5f);
        row_c[r] = rstd;
        row_c[BM + r] = -rstd * mean;
    }

    if constexpr (PH8) {
    // ------------------------------------------------------------------------------------------------------------------
    // Ping-pong K loop (OPT_PINGPONG; the 256x256 tile only), after the CDNA4 guide's "256^2 8-phase template":
    //   * a K-tile is staged as FOUR 16 KiB half-tiles -- B0, A0, B1, A1 -- into 2 x 4 LDS slots (128 KiB as before);
    //     A half h holds the tile rows wm*128 + h*64 + [0,64) of BOTH wave rows, B half g the tile columns
    //     wn*64 + g*32 + [0,32) of all four wave columns, so every wave works on the same half-tiles at the same time
    //     while its own 128 x 64 output block stays contiguous (the epilogue below is unchanged);
    //   * TWO phases per K-tile, two 64 x 32 quadrants of the wave's block (32 MFMAs) each: M1 reads B0, A0, B1 (16 fragment
    //     reads) and runs (A0,B0) (A0,B1); M2 reads A1 (8) and runs (A1,B1) (A1,B0); every phase issues TWO half-tiles of
    //     LDS-DMA (4 instructions per lane).  (r02: the template's FOUR 16-MFMA phases per K-tile ran first -- 12 / 4 / 8 / 0
    //     reads, one half-tile per phase, vmcnt(6); same-process A/B of the two, bit-identical outputs: qkv 334 -> 313 us,
    //     c_fc 478 -> 459, N = 768 shapes equal; end to end generation +1.4 %.  Half the barriers; levelling the four-phase
    //     reads to 8 / 4 / 8 / 4 instead had changed nothing.)
    //   * the half-tiles of the next tiles are issued two phases ahead of their first read and the wait is COUNTED (vmcnt(4)
    //     once per K-tile, in M2, never 0 inside the loop): the two half-tiles just issued stay in flight across the barriers;
    //   * the two wave rows run ONE barrier apart: while wm = 0 issues its MFMAs, wm = 1 reads fragments and issues DMA,
    //     then they swap -- each SIMD holds one wave of either row, so its matrix pipe and its LDS / VMEM issue alternate.
    // Where a K-tile's ~3100 cycles go (r03s, shader-clock stamps of one workgroup, profiles/r03s_gemm_stamps_*.log): per phase and wave, load work
    // (fragment reads + DMA issue + counted wait) 360-600, wait at the mid barrier for the other row's MFMAs 120-400, the 32 MFMAs 590-640
    // (512 back to back), phase-end barrier turn-around ~130: the half-period is MFMA segment + barrier turn-around ~ 770, the load work
    // hides.  Taking the phase-end barrier 3 or 8 MFMAs early (so that the other row is released while this one still feeds the pipe)
    // was bit-identical and 8-10 % SLOWER on every shape (r03s): two rows' MFMAs interleaved on one SIMD cost more than the turn-around.
    // Slot reuse (WAR): every phase retires its fragment reads (lgkmcnt(0)) BEFORE its first barrier, so a half-tile may be
    // restaged one phase after its last read; a staged half-tile is first read one phase after the counted wait + barrier that
    // retires it (RAW) -- the guide's rules for two wave groups staggered by a barrier.
    // ------------------------------------------------------------------------------------------------------------------
    constexpr int SLOT = 16384, KBUF = 4 * SLOT;
    enum { hB0 = 0, hA0 = 1, hB1 = 2, hA1 = 3 };
    unsigned sa8[2][2], sb8[2][2];                      // [half][8-row piece]: byte offset of this lane's source row
    auto source_rows = [&](int tm0, int tn0) {          // ... for the tile at (tm0, tn0)
#pragma unroll
        for (int hf = 0; hf < 2; ++hf)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int lr = wave * 16 + j * 8 + srow;                                    // local row inside the half-tile
                const int ra = tm0 + (lr >> 6) * 128 + hf * 64 + (lr & 63);
                const int rb = tn0 + (lr >> 5) * 64 + hf * 32 + (lr & 31);
                sa8[hf][j] = a_off(ra);
                sb8[hf][j] = src_off(min(rb, a.N - 1), a.ldw);
            }
    };
    source_rows(m0, n0);
    const unsigned smem_lds = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(lptr_t)smem);
    const unsigned wave_lds = (unsigned)__builtin_amdgcn_readfirstlane(wave * 2048);
    auto stage_half = [&](int buf, int which, int kt) {
        const int hf = which >> 1;
        // LDS-DMA as scalar base (the K-tile's) + 32-bit lane offset, from inline asm: hipcc turns the builtin's address into a 64-bit
        // vector add per instruction (v_lshl_add_u64) and the LDS address into two v_readfirstlane -- vector-port instructions of the
        // loading row beside the other row's MFMAs.  Here a DMA instruction costs scalar instructions only (r03w, same-process A/B at
        // M = 151 296: qkv 479 -> 468 us, c_fc 698 -> 691, c_proj 582 -> 578, K loop alone +0.6-1.3 %).  The compiler does not see these
        // loads: every wait for them is one of the counted s_waitcnt of the loop (tests/test_isa_sync_templates.py).
        const char* ak = a_tile(kt);
        const char* wk = (const char*)W + (long)kt * 128;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const unsigned dst = smem_lds + (unsigned)(buf * KBUF + which * SLOT + j * 1024) + wave_lds;   // scalar arithmetic only
            if (which & 1) {
                if constexpr ((OPT & OPT_A_NT) != 0) asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1 nt" :: "v"(sa8[hf][j]), "s"(ak), "s"(dst) : "memory", "m0");
                else asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" :: "v"(sa8[hf][j]), "s"(ak), "s"(dst) : "memory", "m0");
            } else {
                asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" :: "v"(sb8[hf][j]), "s"(wk), "s"(dst) : "memory", "m0");
            }
        }
    };
    const int a_lane = (wm * 64 + fr) * 128, b_lane = (wn * 32 + fr) * 128;
    half8_t fa[4][2], fb0[2][2], fb1[2][2];
    auto read_a = [&](const char* buf, int hf) {
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) {
            fa[ii][0] = *(const half8_t*)(buf + (1 + 2 * hf) * SLOT + a_lane + ii * 2048 + ch0);
            fa[ii][1] = *(const half8_t*)(buf + (1 + 2 * hf) * SLOT + a_lane + ii * 2048 + ch1);
        }
    };
    auto read_b = [&](const char* buf, int g, half8_t (&fb)[2][2]) {
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            fb[jj][0] = *(const half8_t*)(buf + 2 * g * SLOT + b_lane + jj * 2048 + ch0);
            fb[jj][1] = *(const half8_t*)(buf + 2 * g * SLOT + b_lane + jj * 2048 + ch1);
        }
    };
    auto quadrant = [&](int hf, int g, half8_t (&fb)[2][2]) {
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int st = 0; st < 2; ++st)
#pragma unroll
            for (int ii = 0; ii < 4; ++ii)
#pragma unroll
                for (int jj = 0; jj < 2; ++jj)
                    acc[hf * 4 + ii][g * 2 + jj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb[jj][st], fa[ii][st], acc[hf * 4 + ii][g * 2 + jj], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
    };
#define OVMR_PH_END()                                                     \
    __builtin_amdgcn_sched_barrier(0);                                    \
    __builtin_amdgcn_s_barrier();                                         \
    __builtin_amdgcn_sched_barrier(0);
    // Tile loop (LOOPED): the epilogue constants of a tile as a load into registers and, an epilogue later, the arithmetic and the
    // LDS write into constant block `blk` -- the same loads, sums and roundings as the prologue's block below.  The first four
    // statistics slots are loaded at once (predicated); launches with more slots (K > 1024) read the rest at the write.
    float cr[8];
    auto load_consts = [&](int tm0, int tn0) {
#pragma unroll
        for (int q = 0; q < 8; ++q) cr[q] = 0.f;
        if (tid < BN5) {
            const int n = tn0 + tid;
            if (n < a.N) { cr[0] = a.ln_g[n]; cr[1] = a.ln_b[n]; }
        } else {
            const float2_t* sp = (const float2_t*)a.ln_stats + (long)min(tm0 + tid - BN5, a.M - 1) * (a.ln_stride ? a.ln_stride : a.ln_slots);
#pragma unroll
            for (int sl = 0; sl < 4; ++sl)
                if (sl < a.ln_slots) { const float2_t p = sp[sl]; cr[2 * sl] = p[0]; cr[2 * sl + 1] = p[1]; }
        }
    };
    auto store_consts = [&](int blk, int tm0) {
        float* cc = (float*)(smem + 2 * KBUF + blk * V5_CONST_BLOCK);
        if (tid < BN5) {
            cc[tid] = cr[0];
            cc[BN5 + tid] = cr[1];
        } else {
            const int r = tid - BN5;
            const float2_t* sp = (const float2_t*)a.ln_stats + (long)min(tm0 + r, a.M - 1) * (a.ln_stride ? a.ln_stride : a.ln_slots);
            float su = 0.f, sq = 0.f;
#pragma unroll
            for (int sl = 0; sl < 4; ++sl)
                if (sl < a.ln_slots) { su += cr[2 * sl]; sq += cr[2 * sl + 1]; }
            for (int sl = 4; sl < a.ln_slots; ++sl) { const float2_t p = sp[sl]; su += p[0]; sq += p[1]; }
            const float inv_k = 1.0f / (float)a.K;
            const float mean = su * inv_k;
            const float rstd = 1.0f / sqrtf(fmaxf(sq * inv_k - mean * mean, 0.f) + 1e-5f);
            cc[2 * BN5 + r] = rstd;
            cc[2 * BN5 + BM + r] = -rstd * mean;
        }
    };
    // prologue: tile 0 complete, two half-tiles of tile 1 in flight
    stage_half(0, hB0, 0); stage_half(0, hA0, 0); stage_half(0, hB1, 0); stage_half(0, hA1, 0);
    // epilogue constants -> LDS (the compiler waits for their global loads with vmcnt(0), i.e. also for tile 0, which the first
    // phase needs anyway; first read after the K loop)
    if constexpr (LOOPED) {
        load_consts(m0, n0);
        store_consts(0, m0);
    } else
    if (tid < BN5) {
        const int n = n0 + tid;
        float c0 = 0.f, c1 = 0.f;
        if (n < a.N) {
            if (HAS_BIAS) c0 = (float)((const half_t*)a.bias)[n];
            if (LNF) { c0 = a.ln_g[n]; c1 = a.ln_b[n]; }
        }
        col_c[tid] = c0;
        col_c[BN5 + tid] = c1;
    } else if (LNF && tid - BN5 < BM) {
        const int r = tid - BN5;
        const float2_t* sp = (const float2_t*)a.ln_stats + (long)min(m0 + r, a.M - 1) * (a.ln_stride ? a.ln_stride : a.ln_slots);
        float su = 0.f, sq = 0.f;
        for (int sl = 0; sl < a.ln_slots; ++sl) { const float2_t p = sp[sl]; su += p[0]; sq += p[1]; }
        const float inv_k = 1.0f / (float)a.K;
        const float mean = su * inv_k;
        const float rstd = 1.0f / sqrtf(fmaxf(sq * inv_k - mean * mean, 0.f) + 1e-5f);
        row_c[r] = rstd;
        row_c[BM + r] = -rstd * mean;
    }
    __builtin_amdgcn_sched_barrier(0);
    stage_half(1, hB0, 1); stage_half(1, hA0, 1);
    // LOOPED: the tile loop, its body not indented -- dispatch slot `dslot`, constant block `cb`; every other kernel leaves it after the K loop
    for (int dslot = blockIdx.x, cb = 0;; cb ^= 1) {
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (wm == 1) __builtin_amdgcn_s_barrier();          // the second wave row runs one barrier behind the first
    __builtin_amdgcn_sched_barrier(0);
    const char* const bufE = smem;
    const char* const bufO = smem + KBUF;
#define OVMR_P4_MID()                                                     \
    __builtin_amdgcn_sched_barrier(0);                                    \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                    \
    __builtin_amdgcn_s_barrier();                                         \
    __builtin_amdgcn_sched_barrier(0);
    for (int kt = 0; kt < nk; kt += 2) {
        const bool more = kt + 2 < nk;
        // M1 even: stage B1, A1 of the odd tile
        read_b(bufE, 0, fb0);
        read_a(bufE, 0);
        read_b(bufE, 1, fb1);
        __builtin_amdgcn_sched_barrier(0);
        stage_half(1, hB1, kt + 1); stage_half(1, hA1, kt + 1);
        OVMR_P4_MID()
        quadrant(0, 0, fb0);
        quadrant(0, 1, fb1);
        OVMR_PH_END()
        // M2 even: stage B0, A0 of tile kt+2; the odd tile must have landed
        read_a(bufE, 1);
        __builtin_amdgcn_sched_barrier(0);
        if (more) { stage_half(0, hB0, kt + 2); stage_half(0, hA0, kt + 2); }
        __builtin_amdgcn_sched_barrier(0);
        if (more) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        OVMR_P4_MID()
        quadrant(1, 1, fb1);
        quadrant(1, 0, fb0);
        OVMR_PH_END()
        // M1 odd: stage B1, A1 of tile kt+2
        read_b(bufO, 0, fb0);
        read_a(bufO, 0);
        read_b(bufO, 1, fb1);
        __builtin_amdgcn_sched_barrier(0);
        if (more) { stage_half(0, hB1, kt + 2); stage_half(0, hA1, kt + 2); }
        OVMR_P4_MID()
        quadrant(0, 0, fb0);
        quadrant(0, 1, fb1);
        OVMR_PH_END()
        // M2 odd: stage B0, A0 of tile kt+3; tile kt+2 must have landed
        read_a(bufO, 1);
        __builtin_amdgcn_sched_barrier(0);
        if (more) { stage_half(1, hB0, kt + 3); stage_half(1, hA0, kt + 3); }
        __builtin_amdgcn_sched_barrier(0);
        if (more) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        OVMR_P4_MID()
        quadrant(1, 1, fb1);
        quadrant(1, 0, fb0);
        OVMR_PH_END()
    }
#undef OVMR_P4_MID
    if (wm == 0) __builtin_amdgcn_s_barrier();          // balances the extra barrier of the second wave row
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (!LOOPED) break;
    else {
        // ---- the next tile's operands, then this tile's epilogue (header: "Tile loop")
        const int cm0 = m0, cn0 = n0;
        dslot += (int)gridDim.x;
        const bool next = dslot < tiles_m * tiles_n;        // workgroup-uniform
        if (next) {
            v5_tile_of(dslot, tiles_m, tiles_n, a.n_group, tm, tn);
            m0 = tm * BM;
            n0 = tn * BN5;
            source_rows(m0, n0);
            load_consts(m0, n0);
            __builtin_amdgcn_sched_barrier(0);
            stage_half(0, hB0, 0); stage_half(0, hA0, 0); stage_half(0, hB1, 0); stage_half(0, hA1, 0);
            stage_half(1, hB0, 1); stage_half(1, hA0, 1);
            __builtin_amdgcn_sched_barrier(0);
        }
        // Results through LDS in steps of 16 accumulator rows: 16 rows x 64 columns = 2 KiB per wave, behind the constant blocks, so
        // that the K buffers are the next tile's from here on.  Same swizzle, same 16-byte stores of 8 rows x 128 B as the epilogue
        // below.  A step's constants are needed for all four column blocks, so the column constants of the wave's 64 columns are
        // held in 32 registers for the whole epilogue (the fragment registers of the K loop are free here); a row's pair is read
        // once per step.
        half_t* const C = (half_t*)a.C;
        const float* const ccol = (const float*)(smem + 2 * KBUF + cb * V5_CONST_BLOCK);
        const float* const crow = ccol + 2 * BN5;
        char* const et = smem + 2 * KBUF + 2 * V5_CONST_BLOCK + wave * (16 * EP);
        const int er = lane >> 3, nn = cn0 + wn * 64 + (lane & 7) * 8;
        const int rd_off = stage_rd();
        const bool full_tile = cm0 + BM <= a.M && cn0 + BN5 <= a.N;   // workgroup-uniform
        float4_t c0[4], c1[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            c0[j] = *(const float4_t*)(ccol + wn * 64 + j * 16 + fg * 4);
            c1[j] = *(const float4_t*)(ccol + BN5 + wn * 64 + j * 16 + fg * 4);
        }
        // interior tiles (all but the last row / column of tiles) store without bounds compares, as below; each form ends with the
        // next tile's constants, so that the wait hipcc puts in front of them counts that form's own stores and drains none of them
        auto convert_and_store = [&](auto guarded) {
            half_t* dst = C + (long)(cm0 + wm * (BM / 2) + er) * a.ldc + nn;
            const long step = 8L * a.ldc;
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const int r = wm * (BM / 2) + i * 16 + fr;
                const float ln_r = crow[r], ln_t = crow[BM + r];
#pragma unroll
                for (int j = 0; j < 4; ++j) *(half4_t*)(et + stage_wr(j)) = ln_fold4(acc[i][j], ln_r, ln_t, c0[j], c1[j]);
                half8_t vv[2];
#pragma unroll
                for (int it = 0; it < 2; ++it) vv[it] = stage_unswap(*(const half8_t*)(et + it * 8 * EP + rd_off), it);
#pragma unroll
                for (int it = 0; it < 2; ++it, dst += step) {
                    if (decltype(guarded)::value && !(cm0 + wm * (BM / 2) + i * 16 + it * 8 + er < a.M && nn < a.N)) continue;   // N % 8 == 0 is guaranteed by the launcher
                    if (NT) __builtin_nontemporal_store(vv[it], (half8_t*)dst);
                    else *(half8_t*)dst = vv[it];
                }
                __builtin_amdgcn_sched_barrier(0);       // a step's conversions are not hoisted over the step before (registers)
            }
            if (next) store_consts(cb ^ 1, m0);
        };
        if (full_tile) convert_and_store(std::false_type{});
        else convert_and_store(std::true_type{});
        if (!next) return;
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = (float4_t){0.f, 0.f, 0.f, 0.f};
    }
    }
#undef OVMR_PH_END
    } else
    if (OPT & OPT_BOUNDARY) {
    // K loop with the iteration boundary moved INSIDE the MFMA stream.  All of a K-tile's fragment reads are issued two steps
    // before its last MFMAs, so the wait for the next tile's LDS-DMA, the workgroup barrier, the next tile's first six fragment
    // reads and the LDS-DMA issue for the tile after it all happen in front of the last two steps (8 MFMAs per wave): the matrix
    // pipe works through those while the new fragments are in flight, instead of every wave of the CU waiting on LDS at once.
    constexpr int D = 2, R = D + 2;                 // deferred steps / A-fragment ring
    static_assert((2 * MT) % R == 0 && D <= MT, "");
    half8_t fb[2][4], fa[R];
    auto first_reads = [&](const char* buf) {
#pragma unroll
        for (int t = 0; t < 4; ++t) fb[0][t] = *(const half8_t*)(buf + b_row_off + t * 2048 + ch0);
#pragma unroll
        for (int t = 0; t < D; ++t) fa[t] = *(const half8_t*)(buf + a_row_off + (t % MT) * 2048 + (t / MT ? ch1 : ch0));
    };
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    first_reads(smem);
    __builtin_amdgcn_sched_barrier(0);
    if (nk > 1) stage(1, 1);
    __builtin_amdgcn_sched_barrier(0);
    for (int kt = 0; kt < nk; ++kt) {
        const char* cur = smem + (kt & 1) * STAGE;
#pragma unroll
        for (int st = 0; st < 2 * MT - D; ++st) {
            const int nx = st + D;
            fa[nx % R] = *(const half8_t*)(cur + a_row_off + (nx % MT) * 2048 + (nx / MT ? ch1 : ch0));
            if (st == 1) {
#pragma unroll
                for (int t = 0; t < 4; ++t) fb[1][t] = *(const half8_t*)(cur + b_row_off + t * 2048 + ch1);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[st % MT][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb[st / MT][j], fa[st % R], acc[st % MT][j], 0, 0, 0);
        }
#pragma unroll
        for (int st = 0; st < 2 * MT - D; ++st) {
            if (st == 1) __builtin_amdgcn_sched_group_barrier(0x100, 5, 0);
            else __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (kt + 1 < nk) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // tile kt+1 landed (issued one iteration ago)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // every fragment of tile kt is in registers
            __builtin_amdgcn_s_barrier();                          // ... for every wave: buffer kt & 1 is free
            __builtin_amdgcn_sched_barrier(0);
            first_reads(smem + ((kt + 1) & 1) * STAGE);
            __builtin_amdgcn_sched_barrier(0);
            if (kt + 2 < nk) stage(kt & 1, kt + 2);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int st = 2 * MT - D; st < 2 * MT; ++st)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[st % MT][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb[st / MT][j], fa[st % R], acc[st % MT][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
    } else {
    for (int kt = 0; kt < nk; ++kt) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                  // tile kt landed for every wave; buffer (kt+1)&1 is free
        __builtin_amdgcn_sched_barrier(0);
        const char* cur = smem + (kt & 1) * STAGE;
        half8_t fb[2][4], fa[3];
        // software-pipelined fragment reads: A fragment of step t+2 and the B fragments of the next k-step are
        // issued before the MFMAs of step t; sched_group_barrier pins that order for the machine scheduler.
        // The first six reads go out BEFORE the next K-tile's eight LDS-DMA instructions: their LDS latency then runs
        // under the DMA issue (address adds + VMEM issue) instead of after it (same-process A/B: within noise, kept).
#pragma unroll
        for (int t = 0; t < 4; ++t) fb[0][t] = *(const half8_t*)(cur + b_row_off + t * 2048 + ch0);
        fa[0] = *(const half8_t*)(cur + a_row_off + ch0);
        fa[1] = *(const half8_t*)(cur + a_row_off + 2048 + ch0);
        __builtin_amdgcn_sched_barrier(0);
        if (kt + 1 < nk) stage((kt + 1) & 1, kt + 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int st = 0; st < MT; ++st) {
            const int nx = st + 2;
            fa[nx % 3] = *(const half8_t*)(cur + a_row_off + (nx % MT) * 2048 + (nx / MT ? ch1 : ch0));
            if (st == 1) {
#pragma unroll
                for (int t = 0; t < 4; ++t) fb[1][t] = *(const half8_t*)(cur + b_row_off + t * 2048 + ch1);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[st][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb[0][j], fa[st % 3], acc[st][j], 0, 0, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x100, 6, 0);
#pragma unroll
        for (int st = 0; st < MT; ++st) {
            if (st == 1) __builtin_amdgcn_sched_group_barrier(0x100, 5, 0);
            else __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
        }
#pragma unroll
        for (int st = MT; st < 2 * MT; ++st) {
            const int nx = st + 2;
            if (nx < 2 * MT) fa[nx % 3] = *(const half8_t*)(cur + a_row_off + (nx % MT) * 2048 + ch1);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[st - MT][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb[1][j], fa[st % 3], acc[st - MT][j], 0, 0, 0);
        }
#pragma unroll
        for (int st = MT; st < 2 * MT; ++st) {
            if (st + 2 < 2 * MT) __builtin_amdgcn_sched_group_barrier(0x100, 1, 1);
            __builtin_amdgcn_sched_group_barrier(0x008, 4, 1);
        }
    }

    }
    // ---------------------------------------------------------------- epilogue through LDS
    half_t* C = (half_t*)a.C;
    if constexpr (EPI == EPI_SCALE_ARGMAX) {
        // Logits that are never stored: u = h(h(acc) * scale) exactly as EPI_SCALE, then per row the maximum of this tile's
        // columns and the LOWEST column holding it.  A row's 64 columns of one wave sit in four lanes (fg) x 16 values;
        // lanes walk their columns in increasing order, so a strict > keeps the first maximum; lanes and the four column
        // waves are merged with ties to the lower column.
        __syncthreads();                                               // every wave is done with the K buffers
        int* arg_lds = (int*)smem;                                     // [BM rows][4 column waves][value bits, column]
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            float bv = -INFINITY;
            int bc = 0x7fffffff;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c0 = n0 + wn * 64 + j * 16 + fg * 4;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float u = (float)(half_t)((float)(half_t)acc[i][j][r] * a.scale);
                    if (c0 + r < a.N && (u > bv || bc == 0x7fffffff)) { bv = u; bc = c0 + r; }
                }
            }
#pragma unroll
            for (int o = 16; o <= 32; o <<= 1) {
                const float ov = __shfl_xor(bv, o, 64);
                const int oc = __shfl_xor(bc, o, 64);
                if (ov > bv || (ov == bv && oc < bc)) { bv = ov; bc = oc; }
            }
            if (fg == 0) {
                int* d = arg_lds + ((wm * (BM / 2) + i * 16 + fr) * 4 + wn) * 2;
                d[0] = __float_as_int(bv);
                d[1] = bc;
            }
        }
        __syncthreads();
        if (tid < BM && m0 + tid < a.M) {
            float bv = __int_as_float(arg_lds[tid * 8]);
            int bc = arg_lds[tid * 8 + 1];
#pragma unroll
            for (int w = 1; w < 4; ++w) {                               // column waves in increasing column order
                const float v = __int_as_float(arg_lds[tid * 8 + 2 * w]);
                const int vc = arg_lds[tid * 8 + 2 * w + 1];
                if (v > bv || (v == bv && vc < bc)) { bv = v; bc = vc; }
            }
            int* dst = (int*)a.argmax_out + ((long)(m0 + tid) * tiles_n + tn) * 2;
            dst[0] = __float_as_int(bv);
            dst[1] = bc;
        }
        return;
    }
    char* et = smem + wave * (64 * EP);                 // this wave's 64-row x 64-column staging tile
    const int er = lane >> 3, ec = (lane & 7) * 8;     // phase 2: row within an 8-row group, first column
    // The staging tile has 128-byte rows of sixteen 8-byte units; unit u of row r is stored at u ^ f(r & 15),
    // f(r) = ((r & 7) << 1) | (r >> 3): the 16-byte chunk index is XORed with r & 7 (the K loop's swizzle) and the two halves of
    // a chunk trade places in rows 8..15.  Phase 1 (8-byte writes, 16 lanes = the 16 rows of one unit column, 32 banks): f is a
    // bijection, 16 different units = all 32 banks.  Phase 2 reads whole chunks (ds_read_b128, four lanes each of four rows per
    // group, 64 banks): the chunk XOR keeps the two rows that share a bank half on different chunks, and whether a lane's chunk
    // arrives with its halves exchanged is a compile-time fact (rows it*8 + er: odd it), so putting them back costs nothing.
    // SQ_LDS_BANK_CONFLICT = 0 (profiles/r03b_pmc_gemm_v109.json); the 144-byte padded rows this replaces were 2-way on every
    // write and on one read group in four (r02o: 11.7 % of the LDS cycles) -- at equal run time (r03c: -0.3 ... +0.8 %).
    int wr_off[4];                                      // phase 1: byte offset of column block j inside this lane's row fr
#pragma unroll
    for (int j = 0; j < 4; ++j) wr_off[j] = stage_wr(j);
    const int rd_off = stage_rd();
    auto read_staged = [&](int it) -> half8_t {         // rows it*8 + er, this lane's eight columns
        return stage_unswap(*(const half8_t*)(et + it * 8 * EP + rd_off), it);
    };
    const bool emit_stats = EPI == EPI_BIAS_RES && a.stats_out != nullptr;
    const bool full_tile = EPI != EPI_PATCH && m0 + BM <= a.M && n0 + BN5 <= a.N;   // workgroup-uniform
    float* stat_lds = (float*)(smem + 8 * 64 * EP);      // [BM rows][4 column waves][2], behind the staging tiles
#pragma unroll
    for (int h = 0; h < MT / 4; ++h) {
        // The ONLY workgroup barrier of the epilogue: every wave's K-loop fragment reads must be done before staging tiles
        // overwrite the K buffers.  The staging tile itself is private to its wave (LDS executes a wave's instructions in
        // order), so neither the write -> read turn inside a half nor the read -> write turn between the halves needs one;
        // the barriers that used to sit there also drained vmcnt, i.e. made every wave wait for the first half's global
        // stores before converting the second half.
        if (h == 0) __syncthreads();
        // residual rows of this half: requested now, consumed after phase 1 (their latency used to sit in front of every
        // store: ~6 us per 256x256 tile on out_proj / c_proj).  Requesting them earlier -- the first half under the last
        // K-tile's MFMAs (249 VGPRs), or both halves here -- measured 4-7 % SLOWER on out_proj / c_proj.
        half8_t res8[EPI == EPI_BIAS_RES ? 8 : 1];
        if (EPI == EPI_BIAS_RES) {
            const int nn = n0 + wn * 64 + ec;
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const int m = min(m0 + wm * (BM / 2) + h * 64 + it * 8 + er, a.M - 1);
                res8[EPI == EPI_BIAS_RES ? it : 0] = *(const half8_t*)((const half_t*)a.res + (long)m * a.ldres + min(nn, a.N - 8));   // (a nontemporal load here: out_proj +3 %, c_proj equal, r03)
            }
        }
        float ln_rs[LNF ? 4 : 1], ln_ts[LNF ? 4 : 1];   // LNF: rstd and -rstd * mean of this lane's four rows
        if (LNF) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = wm * (BM / 2) + h * 64 + i * 16 + fr;
                ln_rs[LNF ? i : 0] = row_c[r];
                ln_ts[LNF ? i : 0] = row_c[BM + r];
            }
        }
        // column tile outermost: its constants are read from LDS once per half tile (not once per 16x16 accumulator block).
        // (Reading all of them into registers ahead of the h loop measured 4 % SLOWER on the LN-folding kernels: that
        // changed the K loop's register allocation.)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int cc = wn * 64 + j * 16 + fg * 4;
            const float4_t c0 = *(const float4_t*)(col_c + cc);
            float4_t c1 = c0;
            if (LNF) c1 = *(const float4_t*)(col_c + BN5 + cc);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float4_t v = acc[h * 4 + i][j];
                const float ln_r = ln_rs[LNF ? i : 0], ln_t = ln_ts[LNF ? i : 0];
                half4_t o;
                if (LNF) {
                    o = ln_fold4(v, ln_r, ln_t, c0, c1);
                } else {
                    // float2 sums and __builtin_convertvector: v_pk_add_f32 + v_cvt_pk_f16_f32 (round to nearest even), two
                    // elements per instruction; element-wise casts made hipcc emit cvt + pack + alignbit chains (3.8 -> ~1.6
                    // vector instructions per element in this phase)
#pragma unroll
                    for (int r = 0; r < 4; r += 2) {
                        float2_t x2 = {v[r], v[r + 1]};
                        if (HAS_BIAS) x2 += (float2_t){c0[r], c0[r + 1]};
                        if (EPI == EPI_BIAS_QGELU && GFAST) x2 = quick_gelu_f32x2(x2);
                        half2_t u2 = __builtin_convertvector(x2, half2_t);
                        if (EPI == EPI_SCALE) {                                   // h(h(acc) * scale)
                            float2_t y2 = __builtin_convertvector(u2, float2_t);
                            y2 *= a.scale;
                            u2 = __builtin_convertvector(y2, half2_t);
                        }
                        o[r] = u2[0];
                        o[r + 1] = u2[1];
                    }
                    if (EPI == EPI_BIAS_QGELU && !GFAST) o = quick_gelu_h4(o);
                }
                *(half4_t*)(et + i * 16 * EP + wr_off[j]) = o;
            }
        }
        const int nn = n0 + wn * 64 + ec;
        // residual add + row statistics of one 8-column slice (EPI_BIAS_RES); 8 lanes share a row
        auto finish = [&](half8_t v, int it, int row) -> half8_t {
            if (EPI == EPI_BIAS_RES) {
                const half8_t r8 = res8[EPI == EPI_BIAS_RES ? it : 0];
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = (half_t)((float)v[k] + (float)r8[k]);
                if (emit_stats) {                       // statistics of the STORED fp16 row slice
                    // v_dot2_f32_f16 (two fp16 products + fp32 accumulate) and DPP lane exchanges inside the 8-lane
                    // group: 14 instructions where cvt/add chains and ds_bpermute shuffles took ~45 per store
                    float su = 0.f, sq = 0.f;
                    const half2_t one2 = {(half_t)1.f, (half_t)1.f};
#pragma unroll
                    for (int k = 0; k < 8; k += 2) {
                        const half2_t v2 = {v[k], v[k + 1]};
                        su = __builtin_amdgcn_fdot2(v2, one2, su, false);
                        sq = __builtin_amdgcn_fdot2(v2, v2, sq, false);
                    }
                    su += dpp_f32<0xB1>(su); sq += dpp_f32<0xB1>(sq);       // quad_perm [1,0,3,2]: lane ^ 1
                    su += dpp_f32<0x4E>(su); sq += dpp_f32<0x4E>(sq);       // quad_perm [2,3,0,1]: lane ^ 2
                    su += dpp_f32<0x141>(su); sq += dpp_f32<0x141>(sq);     // row_half_mirror: the other quad of the 8
                    if ((lane & 7) == 0)
                        *(float2_t*)(stat_lds + ((wm * (BM / 2) + h * 64 + row) * 4 + wn) * 2) = (float2_t){su, sq};
                }
            }
            return v;
        };
        if (full_tile) {
            // interior tile (all but the last row / column of tiles): the eight LDS reads go out back to back and the stores
            // walk one pointer; the guarded loop below costs 13 instructions and one exposed LDS round trip per store
            half8_t vv[8];
#pragma unroll
            for (int it = 0; it < 8; ++it) vv[it] = read_staged(it);
            half_t* dst = C + (long)(m0 + wm * (BM / 2) + h * 64 + er) * a.ldc + nn;
            const long step = 8L * a.ldc;
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const half8_t v = finish(vv[it], it, it * 8 + er);
                if (NT) __builtin_nontemporal_store(v, (half8_t*)(dst + it * step));
                else *(half8_t*)(dst + it * step) = v;
            }
        } else {
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const int row = it * 8 + er;
                const int m = m0 + wm * (BM / 2) + h * 64 + row;
                if (m < a.M && nn < a.N) {                  // N % 8 == 0 is guaranteed by the launcher
                    half8_t v = finish(read_staged(it), it, row);
                    long crow = m;
                    if (EPI == EPI_PATCH) {
                        const int b = m / a.rows_in, p = m - b * a.rows_in;
                        crow = (long)b * a.rows_out + 1 + p;
                        half8_t p8 = *(const half8_t*)((const half_t*)a.pos + (long)(1 + p) * a.N + nn);
#pragma unroll
                        for (int k = 0; k < 8; ++k) v[k] = (half_t)((float)v[k] + (float)p8[k]);
                    }
                    half8_t* dst = (half8_t*)(C + crow * a.ldc + nn);
                    if (NT) __builtin_nontemporal_store(v, dst);
                    else *dst = v;
                }
            }
        }
    }
    if (emit_stats) {       // one (sum, sum of squares) pair per row and N tile, the four column waves added in fixed order
        // LDS-only barrier: __syncthreads() would also wait for vmcnt(0), i.e. for this tile's global stores to drain
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (tid < BM && m0 + tid < a.M) {
            const float* p = stat_lds + tid * 8;
            const float su = ((p[0] + p[2]) + p[4]) + p[6], sq = ((p[1] + p[3]) + p[5]) + p[7];
            *(float2_t*)(a.stats_out + ((long)(m0 + tid) * tiles_n + tn) * 2) = (float2_t){su, sq};
        }
    }
}

// max_wgs > 0 (the tile-loop instantiations only): at most so many workgroups walk the tiles; 0: one workgroup per tile
template <int EPI, int MT, int OPT>
int launch_v5_k(const GemmArgs& b, int tiles_m, int tiles_n, int max_wgs, hipStream_t s) {
    constexpr int BM = MT * 32;
    constexpr bool LOOPED = v5_tile_loop(EPI, MT, OPT);
    const size_t lds = LOOPED ? (size_t)2 * (BM + BN5) * 128 + 2 * V5_CONST_BLOCK + V5_STAGING : (size_t)2 * (BM + BN5) * 128 + 2 * BN5 * 4 + 2 * BM * 4;
    static_assert(2 * BN5 * 4 + 2 * 256 * 4 == V5_CONST_BLOCK && 8 * 16 * 128 == V5_STAGING, "");
    static bool attr_set[OVMR_MAX_DEVICES] = {};      // the attribute is per device (one process may drive several)
    int dev = 0;
    HIP_CHECK_RET(hipGetDevice(&dev));
    if (dev >= 0 && dev < OVMR_MAX_DEVICES && !attr_set[dev]) {
        HIP_CHECK_RET(hipFuncSetAttribute((const void*)gemm_f16_v5_kernel<EPI, MT, OPT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_set[dev] = true;
    }
    const int tiles = tiles_m * tiles_n, grid = LOOPED && max_wgs > 0 ? std::min(tiles, max_wgs) : tiles;
    hipLaunchKernelGGL((gemm_f16_v5_kernel<EPI, MT, OPT>), dim3(grid), dim3(512), lds, s, b, tiles_m, tiles_n);
    return (int)hipGetLastError();
}

// Every instantiation gemm_f16_route can ask for, and no other: X(epilogue, MT, OPT).  The ping-pong loop exists for MT = 8 only;
// F: the bits every entry of the group carries.  Residual projections: never the store hint; the boundary loop (K >= 2048) and the
// nontemporal A stream.  LayerNorm fold: the boundary loop wherever the ping-pong loop does not run.  The argmax stores no C.
#define V5_DOUBLE_PP(X, E, F) X(E, 4, (F)) X(E, 8, (F)) X(E, 8, (F) | OPT_PINGPONG)
#define V5_BOUNDARY(X, E, F) X(E, 4, (F) | OPT_BOUNDARY) X(E, 8, (F) | OPT_BOUNDARY)
#define V5_STORES(X, LOOPS, E, F) LOOPS(X, E, (F)) LOOPS(X, E, (F) | OPT_NT_STORE)
#define V5_BOUNDARY_PP(X, E, F) V5_BOUNDARY(X, E, F) X(E, 8, (F) | OPT_PINGPONG)
#define V5_TABLE(X)                                                                                                                \
    V5_STORES(X, V5_DOUBLE_PP, EPI_NONE, 0) V5_STORES(X, V5_DOUBLE_PP, EPI_BIAS, 0)                                                 \
    V5_STORES(X, V5_DOUBLE_PP, EPI_PATCH, 0) V5_STORES(X, V5_DOUBLE_PP, EPI_SCALE, 0)                                               \
    V5_STORES(X, V5_DOUBLE_PP, EPI_BIAS_QGELU, 0) V5_STORES(X, V5_DOUBLE_PP, EPI_BIAS_QGELU, OPT_GELU_F32)                          \
    V5_DOUBLE_PP(X, EPI_BIAS_RES, 0) V5_DOUBLE_PP(X, EPI_BIAS_RES, OPT_A_NT) V5_BOUNDARY(X, EPI_BIAS_RES, 0) V5_BOUNDARY(X, EPI_BIAS_RES, OPT_A_NT) \
    V5_STORES(X, V5_BOUNDARY_PP, EPI_LN_BIAS, 0) V5_DOUBLE_PP(X, EPI_SCALE_ARGMAX, 0)                                               \
    V5_STORES(X, V5_BOUNDARY_PP, EPI_LN_BIAS_QGELU, 0) V5_STORES(X, V5_BOUNDARY_PP, EPI_LN_BIAS_QGELU, OPT_GELU_F32)

}  // namespace

int launch_gemm_f16_v5(const GemmArgs& a, const GemmPlan& p, hipStream_t s, int max_wgs) {
    const int mt = p.tile_rows / 32, tiles_m = (a.M + p.tile_rows - 1) / p.tile_rows, tiles_n = (a.N + BN5 - 1) / BN5;
    const int opt = (p.a_nt ? OPT_A_NT : 0) | (p.loop == LOOP_BOUNDARY ? OPT_BOUNDARY : 0) | (p.loop == LOOP_PINGPONG ? OPT_PINGPONG : 0) |
                    (p.nt_store ? OPT_NT_STORE : 0) | (p.gelu_mode ? OPT_GELU_F32 : 0);
    // GemmPlan::persist: one workgroup per CU (the count is cached per device), or fewer where the caller caps them (max_wgs > 0: tests)
    int wgs = 0;
    if (p.persist) {
        static int n_cu[OVMR_MAX_DEVICES] = {};
        int dev = 0;
        HIP_CHECK_RET(hipGetDevice(&dev));
        if (dev < 0 || dev >= OVMR_MAX_DEVICES) return -100;
        if (!n_cu[dev]) HIP_CHECK_RET(hipDeviceGetAttribute(&n_cu[dev], hipDeviceAttributeMultiprocessorCount, dev));
        wgs = std::max(1, n_cu[dev]);
        if (max_wgs > 0) wgs = std::min(wgs, max_wgs);
    }
#define X(E, MT, OPT) if (a.epi == E && mt == MT && opt == (OPT)) return launch_v5_k<E, MT, (OPT)>(a, tiles_m, tiles_n, wgs, s);
    V5_TABLE(X)
#undef X
    return -3;
}

// The tile loop's walk, for tests/test_gemm_persist_route_cpu.py (no GPU): workgroup by workgroup of a grid of `grid`, the tiles it
// computes in the order it computes them, as (workgroup, tm, tn) triples; returns their number (tiles_m * tiles_n), writes at most `cap`.
extern "C" int ovmr_debug_gemm_tile_walk(int tiles_m, int tiles_n, int n_group, int grid, int* out, int cap) {
    if (tiles_m < 1 || tiles_n < 1 || grid < 1 || !out) return -1;
    int n = 0;
    for (int w = 0; w < grid; ++w)
        for (int slot = w; slot < tiles_m * tiles_n; slot += grid, ++n)
            if (n < cap) {
                out[3 * n] = w;
                v5_tile_of(slot, tiles_m, tiles_n, n_group, out[3 * n + 1], out[3 * n + 2]);
            }
    return n;
}

// (epilogue, MT, OPT) of every entry of the table, for tests/test_gemm_route_cpu.py: returns their number, writes at most `cap`.
extern "C" int ovmr_debug_gemm_tile_kernels(int* out, int cap) {
    int n = 0;
#define X(E, MT, OPT) if (n < cap) { out[3 * n] = E; out[3 * n + 1] = MT; out[3 * n + 2] = (OPT); } ++n;
    V5_TABLE(X)
#undef X
    return n;
}
