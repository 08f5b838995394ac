// Attention variant 3 (fp16, hd = 64, non-causal, 192 < L <= 208: the ViT-B/16 image tower, L = 197): ONE PASS over the keys.
//
// Variants 0 / 1 are flash-style: 64-key blocks, an online softmax whose running maximum / rescale / row-sum state is carried
// from block to block, one workgroup barrier per block.  At L = 197 that machinery buys nothing -- a 16-row query tile against
// ALL 13 key sub-tiles is only 52 score registers per lane -- and it costs: profiles/r02f_pmc_attn.json shows variant 1 neither
// MFMA- nor VALU-issue-bound (matrix pipe 24 % busy, VALU 57 %) but waiting: 33 % of the wave cycles in s_waitcnt / barriers
// and 37 % in issue stalls of short dependent chains.  Here
//   * PERSISTENT: one 14-wave workgroup per CU walks the (image, head) pairs.  K and V of a head (13 x 16 rows x 128 B each,
//     52 KiB) are brought into LDS once by LDS-DMA (source-side XOR swizzle as in variant 1) into one of TWO buffers: the next
//     head streams in under the current head's arithmetic; ONE barrier per head.  (A first version with one 7-wave workgroup
//     per head, 2 per CU, ran at 154 us against 162 for variant 1: load and compute phases of comparable length, half hidden.)
//   * wave w takes query tile w of the head (13 tiles, the 14th wave only helps staging); the tile body (tile() below):
//     26 MFMAs give the whole S^T row block, the EXACT row maximum (no running maximum, no rescale branch), 52 exponentials,
//     P^T packed to fp16 straight into the B operands of the 7 PV steps, V^T through ds_read_b64_tr_b16, the row sum from the
//     matrix pipe, output rows exchanged between lanes so that a store instruction writes 64 contiguous bytes per row;
//   * 14 waves per CU at <= 128 VGPRs (3.5 per SIMD).
// What bounds it (r02m, timing-only ablations of the retired variant 4 -- the same tile body with free-running waves instead of the
// workgroup barrier, last present at a19fe7d): the memory system.  At
// 512 x 12 heads x 197 the kernel moves 620 MB (Q, K, V once in, O once out) in 135-141 us = 4.4-4.6 TB/s; without the output
// stores it takes 108-111 us, streaming K / V alone 55 us (5.6 TB/s), and the tile body hardly matters (no exponentials -4 us,
// no LDS reads -18, one PV MFMA per step -11).  Pinned instruction order, free-running waves, a third buffer and
// head-major strides all land within +-3 % of this kernel.
// Other shapes (text, the CLS-only last block, ViT-L) stay on variants 0 / 1.
#include "attn_common.h"

#include <algorithm>

namespace {

using attn::tr_read;

// One 16-row query tile against ALL keys of a head in LDS.  LDS image of a head: K rows then V rows, 128-byte rows, 16-byte chunk c
// of row r stored in slot c ^ (r & 7).  Lane (fr, fg) of the wave holds query fr of the tile; S^T = K Q^T puts keys on the
// accumulator rows, so a query's scores sit in four lanes (fg) x NT x 4 registers, P^T goes straight into the B operands of the PV
// products, V^T comes through ds_read_b64_tr_b16 and the row sums come from the matrix pipe (ones . P^T).  The instruction order is
// hipcc's: a pinned order (fragment reads run ahead of the MFMAs, the PV steps fenced) measured within +-3 % (file header, r02m).
// o[dt][r]: un-normalised O^T (d = dt*16 + fg*4 + r) of this lane's query; returns the row sum
template <int NT>
__device__ __forceinline__ float tile(const half_t* sK, const half_t* sV, const half8_t (&qf)[2], int L, float scale_log2e,
                                      int fr, int fg, float4_t (&o)[4]) {
    constexpr int NS = (NT + 1) / 2;
    constexpr bool odd_tail = (NT & 1) != 0;
    const float4_t zero = {0.f, 0.f, 0.f, 0.f};
    const int c0 = (fg ^ (fr & 7)) << 3, c1 = ((4 + fg) ^ (fr & 7)) << 3;
    half8_t ones;
#pragma unroll
    for (int j = 0; j < 8; ++j) ones[j] = (half_t)1.f;

    // ---- S^T = K Q^T for all keys: lane (fr, fg) holds query fr, keys nt*16 + fg*4 + r
    float4_t s[NT];
    {
        half8_t kf[NT][2];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            kf[nt][0] = *(const half8_t*)(sK + (nt * 16 + fr) * 64 + c0);
            kf[nt][1] = *(const half8_t*)(sK + (nt * 16 + fr) * 64 + c1);
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            s[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[nt][0], qf[0], zero, 0, 0, 0);
            s[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[nt][1], qf[1], s[nt], 0, 0, 0);
        }
    }
    // V^T fragments of one 32-key step
    auto read_v = [&](int s2, half4_t (&v0)[4], half4_t (&v1)[4]) {
        const bool two = !(odd_tail && s2 == NS - 1);          // the last step of an odd NT holds one sub-tile
        const int kr = attn::vt_row(s2 * 32, fr, fg);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            const int off = attn::vt_col(kr, dt, fr);
            v1[dt] = (half4_t){(half_t)0.f, (half_t)0.f, (half_t)0.f, (half_t)0.f};
            v0[dt] = tr_read(sV + kr * 64 + off);
            if (two) v1[dt] = tr_read(sV + (kr + 16) * 64 + off);
        }
    };
    half4_t v0[4], v1[4];
    {   // keys past L (only in the last sub-tile): -inf
        const int thr = L - (NT - 1) * 16 - fg * 4;
#pragma unroll
        for (int r = 0; r < 4; ++r) s[NT - 1][r] = (r < thr) ? s[NT - 1][r] : -INFINITY;
    }
    // ---- exact row maximum, exponentials against it (raw-score domain: p = exp2(s * c - max * c), c = hd^-0.5 * log2 e)
    float mx = s[0][0];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[nt][r]);
    mx = attn::row_max4(mx);
    const float m_ref = mx * scale_log2e;
    // ---- O^T = V^T P^T in steps of 32 keys; row sums = ones . P^T on the matrix pipe
    float4_t ol = zero;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = zero;
#pragma unroll
    for (int s2 = 0; s2 < NS; ++s2) {
        const bool two = !(odd_tail && s2 == NS - 1);
        read_v(s2, v0, v1);
        half8_t pf;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            pf[j] = (half_t)__builtin_amdgcn_exp2f(__builtin_fmaf(s[2 * s2][j], scale_log2e, -m_ref));
            pf[4 + j] = two ? (half_t)__builtin_amdgcn_exp2f(__builtin_fmaf(s[two ? 2 * s2 + 1 : 0][j], scale_log2e, -m_ref)) : (half_t)0.f;
        }
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            const half8_t vf = {v0[dt][0], v0[dt][1], v0[dt][2], v0[dt][3], v1[dt][0], v1[dt][1], v1[dt][2], v1[dt][3]};
            o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf, o[dt], 0, 0, 0);
        }
        ol = __builtin_amdgcn_mfma_f32_16x16x32_f16(ones, pf, ol, 0, 0, 0);
    }
    return ol[0];                                              // every d-row of ones . P^T holds the row sum of this lane's query
}

// Normalise and store one query row per lane quartet.  The accumulator layout leaves lane (fr, fg) with d = dt*16 + fg*4 + [0,4)
// for dt = 0..3: stored as it is (attn::store_row4), a wave instruction writes 8 bytes per lane, 32-byte pieces of 16 different rows
// (r02m: the 155 MB of output then cost 50 us of a 160 us kernel -- no stores 108 us, these stores 160, 64-byte pieces 138, whole
// rows 137).  One v_permlane16_swap stage per register pair exchanges the dt parity with the lane's fg parity: lane (fr, fg) then
// holds the octets d0 + [0,8) and 32 + d0 + [0,8), d0 = (fg & 1)*16 + (fg >> 1)*8, i.e. 16 contiguous bytes per lane and 64
// contiguous bytes per row in each of the two store instructions.
__device__ __forceinline__ void store_row(half_t* row, const float4_t (&o)[4], float inv, int fg) {
    unsigned w[4][2];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        const half2_t lo = {(half_t)(o[dt][0] * inv), (half_t)(o[dt][1] * inv)}, hi = {(half_t)(o[dt][2] * inv), (half_t)(o[dt][3] * inv)};
        w[dt][0] = __builtin_bit_cast(unsigned, lo);
        w[dt][1] = __builtin_bit_cast(unsigned, hi);
    }
    typedef unsigned uint4v __attribute__((ext_vector_type(4)));
    uint4v a, b;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        auto p = __builtin_amdgcn_permlane16_swap(w[0][k], w[1][k], false, false);
        auto q = __builtin_amdgcn_permlane16_swap(w[2][k], w[3][k], false, false);
        a[k] = (unsigned)p[0]; a[2 + k] = (unsigned)p[1];
        b[k] = (unsigned)q[0]; b[2 + k] = (unsigned)q[1];
    }
    const int d0 = (fg & 1) * 16 + (fg >> 1) * 8;
    *(uint4v*)(row + d0) = a;
    *(uint4v*)(row + 32 + d0) = b;
}

template <int NT>                                      // key sub-tiles of 16: (NT - 1) * 16 < L <= NT * 16
__global__ __launch_bounds__(896, 4) void attn_f16_v3(const half_t* __restrict__ qkv, half_t* __restrict__ out,
                                                      int L, int H, int nBH, float scale_log2e) {
    constexpr int ROWS = NT * 16, NW = 14, NS = (NT + 1) / 2;    // NS: PV steps of 32 keys
    constexpr int HEAD = 2 * ROWS * 64;                         // halves per buffer: K rows, then V rows
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];   // [2 buffers][K | V][ROWS][64]: 128-byte rows, chunk c of row r in slot c ^ (r & 7)
    half_t* smem = (half_t*)smem_raw;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fg = lane >> 4;
    const int D = H * 64, ld = 3 * D;
    const int srow = lane >> 3, schunk = ((lane & 7) ^ srow) * 8;
    const bool has_tile = wave * 16 < L;                       // NT tiles, NW >= NT waves: wave w owns query tile w

    auto head_base = [&](int bh) { return qkv + (long)(bh / H) * L * ld + (bh % H) * 64; };
    // 4 * NT LDS-DMA instructions of 8 rows x 128 B per head, dealt round-robin to the waves
    const unsigned lds_base = (unsigned)(uintptr_t)(attn::lptr_t)smem;
    auto stage = [&](int buf, const half_t* base) {
        for (int ins = wave; ins < 4 * NT; ins += NW) {
            const int isv = ins >= 2 * NT, r0 = (isv ? ins - 2 * NT : ins) * 8;
            const int kc = min(r0 + srow, L - 1);              // rows past the last key repeat it: finite values, masked below
            const unsigned dst = __builtin_amdgcn_readfirstlane(lds_base + 2u * (unsigned)(buf * HEAD + isv * (ROWS * 64) + r0 * 64));
            attn::glds16_asm(base + (1 + isv) * D + (long)kc * ld + schunk, dst);
        }
    };
    auto load_q = [&](const half_t* base, half8_t (&q)[2]) {
        const int qc = min(wave * 16 + fr, L - 1);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) q[ks] = *(const half8_t*)(base + (long)qc * ld + ks * 32 + fg * 8);
    };

    int bh = blockIdx.x;
    if (bh >= nBH) return;
    half8_t qf[2], qn[2];
    stage(0, head_base(bh));
    load_q(head_base(bh), qf);
    for (int it = 0; bh < nBH; ++it, bh += gridDim.x) {
        const int cur = it & 1;
        // this head's K / V (and the query rows) have landed for every wave, and every wave is done with the other buffer
        // (the builtin form, so that hipcc's own scoreboard knows the query loads are back: after an asm wait it re-waited
        // vmcnt(0) -- i.e. for the NEXT head's stream -- in front of the first MFMA)
        __builtin_amdgcn_s_waitcnt(0x0F70);                    // vmcnt(0)
        __syncthreads();
        const int nxt = bh + (int)gridDim.x;
        if (nxt < nBH) {                                       // the next head streams in under this head's arithmetic
            stage(cur ^ 1, head_base(nxt));
            load_q(head_base(nxt), qn);
        }
        if (has_tile) {
            const half_t* sK = smem + cur * HEAD;
            const half_t* sV = sK + ROWS * 64;
            float4_t o[4];
            const float lsum = tile<NT>(sK, sV, qf, L, scale_log2e, fr, fg, o);
            const int qrow = wave * 16 + fr;
            if (qrow < L) {
                const float inv = 1.0f / lsum;
                store_row(out + ((long)(bh / H) * L + qrow) * D + (bh % H) * 64, o, inv, fg);
            }
        }
        qf[0] = qn[0];
        qf[1] = qn[1];
    }
}

}  // namespace

int attn::launch_attention_f16_v3(const half_t* qkv, half_t* out, int B, int L, int H, hipStream_t s) {
    if (!attn::v3_takes(L, L, 0)) return -2;
    constexpr int NT = 13;
    const size_t lds = (size_t)2 * 2 * NT * 16 * 64 * sizeof(half_t);             // two (K | V) buffers: 104 KiB
    static bool attr_set[OVMR_MAX_DEVICES] = {};
    static int n_cu[OVMR_MAX_DEVICES] = {};
    int dev = 0;
    HIP_CHECK_RET(hipGetDevice(&dev));
    if (dev < 0 || dev >= OVMR_MAX_DEVICES) return -100;        // no slot in the tables above: the caller runs variant 1
    if (!attr_set[dev]) {
        HIP_CHECK_RET(hipFuncSetAttribute((const void*)attn_f16_v3<NT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        HIP_CHECK_RET(hipDeviceGetAttribute(&n_cu[dev], hipDeviceAttributeMultiprocessorCount, dev));
        attr_set[dev] = true;
    }
    const int nBH = B * H;
    const int grid = std::min(nBH, std::max(1, n_cu[dev]));     // persistent: one 14-wave workgroup per CU walks the heads
    hipLaunchKernelGGL((attn_f16_v3<NT>), dim3((unsigned)grid), dim3(896), lds, s, qkv, out, L, H, nBH, attn::SCALE_LOG2E);
    return (int)hipGetLastError();
}

