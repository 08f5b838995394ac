// Scaled-dot-product self attention for hd = 64 heads (nn.MultiheadAttention as used at
// clip/model.py:171,184-188): softmax(q k^T / sqrt(hd) + mask) v per (sequence, head).
//
// fp16 kernel (image tower: L = 197/577 no mask; text tower: L <= 77 causal):
//   * one workgroup = up to four 16-row query tiles (one per wave) of one (sequence, head);
//     key/value blocks of 64 keys are staged in LDS and shared by the four waves;
//   * both products are issued "swapped" so the query index always sits on the MFMA lane
//     (lane & 15): S^T = K Q^T, then O^T = V^T P^T.  The row max / row sum are then two
//     shuffles (xor 16, 32), P never leaves registers (the S^T accumulator IS the P^T operand
//     under a key permutation that the V^T fragment mirrors), and the online-softmax rescale of
//     O^T is lane local;
//   * V is transposed while it is staged ([d][key] rows of 136 B, conflict-free ds_read_b64);
//     K rows are XOR-swizzled 128-byte rows (conflict-free ds_read_b128).
// fp32 kernel (aggregator, sequences of n_ctx + shots <= 128 rows, equal or each its own): one thread per query row, K/V in LDS.
#include "attn_common.h"
#include "../../include/ovmr_hip.h"

namespace {

constexpr int KB = 64;      // keys per block
constexpr int VT_LD = 68;   // halves per V^T row (64 keys + 4 pad -> 136 B)

template <bool CAUSAL>
__global__ __launch_bounds__(256) void attn_f16_v0(const half_t* __restrict__ qkv, half_t* __restrict__ out,
                                                   int L, int Lq, int H, int nT, int nWG, float scale_log2e) {
    // Lq <= L: only the first Lq query rows of every sequence are computed, output rows are b*Lq + q
    __shared__ __attribute__((aligned(16))) half_t sK[KB * 64];
    __shared__ __attribute__((aligned(16))) half_t sVt[64 * VT_LD];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fg = lane >> 4;
    const int D = H * 64, ld = 3 * D;
    const int wg = blockIdx.x % nWG, bh = blockIdx.x / nWG;
    const int h = bh % H, b = bh / H;
    const int t0 = (wg * nT) / nWG, t1 = ((wg + 1) * nT) / nWG;
    const int qt = t0 + wave;
    const bool active = qt < t1;
    const half_t* base = qkv + (long)b * L * ld + h * 64;
    const int q = qt * 16 + fr;
    const int qc = min(q, Lq - 1);     // a spare row repeats the last query, never a Q slot behind it (unwritten where Lq < L)

    half8_t qf[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) qf[ks] = *(const half8_t*)(base + (long)qc * ld + ks * 32 + fg * 8);

    float m_run = -INFINITY, l_run = 0.f;
    float4_t o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = (float4_t){0.f, 0.f, 0.f, 0.f};

    const int kmax = CAUSAL ? min(L, t1 * 16) : L;
    for (int k0 = 0; k0 < kmax; k0 += KB) {
        __syncthreads();
        // ---- stage K block (64 keys x 128 B)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int id = tid + 256 * i, key = id >> 3, c = id & 7;
            const int kc = min(k0 + key, L - 1);
            uint4 v = *(const uint4*)(base + D + (long)kc * ld + c * 8);
            *(uint4*)(sK + key * 64 + ((c ^ (key & 7)) << 3)) = v;
        }
        // ---- stage V block transposed: thread = (4 keys) x (4 d)
        {
            const int dg = tid & 15, kg = tid >> 4;
            half4_t r[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int kc = min(k0 + kg * 4 + i, L - 1);
                r[i] = *(const half4_t*)(base + 2 * D + (long)kc * ld + dg * 4);
            }
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                half4_t w = {r[0][d], r[1][d], r[2][d], r[3][d]};
                *(half4_t*)(sVt + (dg * 4 + d) * VT_LD + kg * 4) = w;
            }
        }
        __syncthreads();

        if (active && (!CAUSAL || k0 <= qt * 16 + 15)) {
            float4_t s[4];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                s[nt] = (float4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    half8_t kf = *(const half8_t*)(sK + (nt * 16 + fr) * 64 + ((((ks << 2) + fg) ^ (fr & 7)) << 3));
                    s[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[ks], s[nt], 0, 0, 0);
                }
            }
            float mx = -INFINITY;
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = k0 + nt * 16 + fg * 4 + r;
                    const bool ok = (key < L) && (!CAUSAL || key <= q);
                    const float v = ok ? s[nt][r] * scale_log2e : -INFINITY;
                    s[nt][r] = v;
                    mx = fmaxf(mx, v);
                }
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float m_new = fmaxf(m_run, mx);
            const float alpha = exp2f(m_run - m_new);
            const float psum = attn::exp_sum<4>(s, m_new);
            l_run = l_run * alpha + psum;
            m_run = m_new;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) o[dt] *= alpha;
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                half8_t pf;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    pf[j] = (half_t)s[2 * s2][j];
                    pf[4 + j] = (half_t)s[2 * s2 + 1][j];
                }
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    const half_t* vr = sVt + (dt * 16 + fr) * VT_LD + s2 * 32 + fg * 4;
                    half4_t v0 = *(const half4_t*)vr;
                    half4_t v1 = *(const half4_t*)(vr + 16);
                    half8_t vf = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
                    o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf, o[dt], 0, 0, 0);
                }
            }
        }
    }
    if (active && q < Lq) {
        const float inv = 1.0f / l_run;
        attn::store_row4(out + ((long)b * Lq + q) * D + h * 64 + fg * 4, o, inv);
    }
}

// fp32, sequences of at most 128 rows packed row after row (AggSeqs, common.h): one workgroup per (sequence, head), K and V in LDS sized
// by the launch's longest sequence (q.len rows each), a thread per query row through the three steps of attn::F32Row, single-pass online
// softmax.  A row's bits depend on its own sequence alone.  TABLE: the starts come from the device prefix sum, clamped, and a workgroup
// takes at most q.len rows; uniform: sequence b is the rows [b * q.len, (b + 1) * q.len), nothing loaded.
template <bool TABLE>
__global__ __launch_bounds__(128) void attn_f32_small(const float* __restrict__ qkv, float* __restrict__ out, const AggSeqs q,
                                                      int H, float scale) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* sK = sm;
    float* sV = sm + q.len * 64;
    const int tid = threadIdx.x;
    const int h = blockIdx.x % H, b = blockIdx.x / H;
    const int D = H * 64, ld = 3 * D;
    const long r0 = q.start<TABLE>(b);
    const int L = TABLE ? (int)min(max(q.start<TABLE>(b + 1) - r0, 0L), (long)q.len) : q.len;
    const float* base = qkv + r0 * ld + h * 64;
    for (int i = tid; i < L * 16; i += blockDim.x) {
        const int row = i >> 4, c = i & 15;
        *(float4_t*)(sK + row * 64 + c * 4) = *(const float4_t*)(base + D + (long)row * ld + c * 4);
        *(float4_t*)(sV + row * 64 + c * 4) = *(const float4_t*)(base + 2 * D + (long)row * ld + c * 4);
    }
    __syncthreads();
    if (tid >= L) return;
    attn::F32Row r;
    attn::f32_row_begin(r, base + (long)tid * ld);
    attn::f32_row_keys(r, sK, sV, 0, L, scale);
    attn::f32_row_end(r, out + (r0 + tid) * D + h * 64);
}

// The same attention over sequences of any length up to q.len, in the same two modes: a workgroup is the 128-row query tile `tile` of one
// (sequence, head), a thread per query row, and walks the sequence's keys IN ORDER in blocks of attn::F32_KEYS keys staged in LDS --
// stage, barrier, every live row advances over the block's keys, barrier, next block.  The rows go through the same three steps as
// attn_f32_small's, the keys in the same order: a sequence of at most 128 rows gets the bits that kernel gives it, a longer one the
// bits of this kernel on it alone, and q.len, which only sizes the grid (nT = ceil(q.len / 128) tiles per (sequence, head)), changes
// nothing.
// Barriers: L and `tile` are the same for every thread of a workgroup, so the return of a tile that starts at or behind the sequence's
// end is taken by all of them or by none, in front of the first barrier, and the block loop has the same trip count for all.  A
// thread whose row lies behind the end (the last tile) stages and meets every barrier; it only skips the steps of its row.
template <bool TABLE>
__global__ __launch_bounds__(128) void attn_f32_long(const float* __restrict__ qkv, float* __restrict__ out, const AggSeqs q, int H,
                                                     int nT, float scale) {
    constexpr int TILE = attn::F32_TILE, KEYS = attn::F32_KEYS;
    __shared__ __attribute__((aligned(16))) float sK[KEYS * 64], sV[KEYS * 64];
    const int tid = threadIdx.x;
    const int tile = blockIdx.x % nT, bh = blockIdx.x / nT;
    const int h = bh % H, b = bh / H;
    const int D = H * 64, ld = 3 * D;
    const long r0 = q.start<TABLE>(b);
    const int L = TABLE ? (int)min(max(q.start<TABLE>(b + 1) - r0, 0L), (long)q.len) : q.len;
    if (tile * TILE >= L) return;                            // workgroup-uniform, before any barrier
    const int row = tile * TILE + tid;
    const bool live = row < L;
    const float* base = qkv + r0 * ld + h * 64;
    attn::F32Row r;
    if (live) attn::f32_row_begin(r, base + (long)row * ld);
    for (int k0 = 0; k0 < L; k0 += KEYS) {
        const int n = min(KEYS, L - k0);
        const float* kb = base + (long)k0 * ld;
        for (int i = tid; i < n * 16; i += TILE) {
            const int kr = i >> 4, c = i & 15;
            *(float4_t*)(sK + kr * 64 + c * 4) = *(const float4_t*)(kb + D + (long)kr * ld + c * 4);
            *(float4_t*)(sV + kr * 64 + c * 4) = *(const float4_t*)(kb + 2 * D + (long)kr * ld + c * 4);
        }
        __syncthreads();
        if (live) attn::f32_row_keys(r, sK, sV, 0, n, scale);
        __syncthreads();                                     // the block is read before the next one overwrites it
    }
    if (live) attn::f32_row_end(r, out + (r0 + row) * D + h * 64);
}

// Which kernel a launch of `variant` runs: 0 attn_f16_v0, 1 attn_f16_v1, 2 attn_f16_short, 3 attn_f16_v3, 5 attn_f16_v5
// (include/ovmr_hip.h, "attn").  Every kernel computes the same values: a mistake here costs time, not correctness, and only
// tests/test_attn_route_cpu.py would see it.
enum Kernel { K_V0 = 0, K_V1 = 1, K_SHORT = 2, K_V3 = 3, K_V5 = 5 };

Kernel route(int variant, int L, int Lq, int causal) {
    if (variant >= 1 && attn::short_takes(L, Lq)) return K_SHORT;
    if (variant == 4) variant = 3;    // 4: the number of a retired kernel, an alias of 3 so that the option value keeps its meaning
    if (variant == 3 && attn::v3_takes(L, Lq, causal)) return K_V3;
    if ((variant == 3 || variant == 5) && attn::v5_takes(L, Lq, causal)) return K_V5;
    if ((variant == 1 || variant == 3 || variant == 5) && attn::v1_wanted(L)) return K_V1;
    return K_V0;
}

// Which fp32 kernel a launch whose longest sequence has `len` rows runs.  `cap` is the largest length the caller lets through: 128 from
// the debug hooks of attn_f32_small, option "agg_max_len" from the generator, OVMR_AGG_MAX_LEN_CEILING at the most.  Up to 128 rows the
// launch is attn_f32_small's, as it always was; a longer one runs attn_f32_long for ALL its sequences, the short ones to the same bits.
enum F32Kernel { F32_REFUSED, F32_SMALL, F32_LONG };

F32Kernel route_f32(int len, int cap) {
    if (len < 1 || len > cap || len > OVMR_AGG_MAX_LEN_CEILING) return F32_REFUSED;
    return len <= attn::F32_SMALL_MAX ? F32_SMALL : F32_LONG;
}

}  // namespace

extern "C" int ovmr_debug_attention_route(int variant, int L, int Lq, int causal) { return route(variant, L, Lq, causal); }

int launch_attention_f16(const half_t* qkv, half_t* out, int B, int L, int H, int causal, int variant, hipStream_t s) {
    return launch_attention_f16_q(qkv, out, B, L, L, H, causal, variant, s);
}

int launch_attention_f16_q(const half_t* qkv, half_t* out, int B, int L, int Lq, int H, int causal, int variant, hipStream_t s) {
    if (B <= 0 || L <= 0 || Lq <= 0) return 0;
    if (Lq > L) return -2;
    switch (route(variant, L, Lq, causal)) {
    case K_SHORT: {
        const long row0 = 0;
        return launch_attention_f16_short(qkv, out, 1, &B, &L, &row0, H, causal, s);
    }
    case K_V3:
        if (const int rc = attn::launch_attention_f16_v3(qkv, out, B, L, H, s); rc != -100) return rc;
        [[fallthrough]];              // -100: no slot for this device in the launcher's table; the launch runs as variant 1
    case K_V1: return attn::launch_attention_f16_v1(qkv, out, B, L, Lq, H, causal, s);
    case K_V5: return attn::launch_attention_f16_v5(qkv, out, B, L, Lq, H, s);
    case K_V0: break;
    }
    const int nT = (Lq + 15) / 16, nWG = (nT + 3) / 4;
    const dim3 grid((unsigned)((long)B * H * nWG));
    if (causal) hipLaunchKernelGGL(attn_f16_v0<true>, grid, dim3(256), 0, s, qkv, out, L, Lq, H, nT, nWG, attn::SCALE_LOG2E);
    else hipLaunchKernelGGL(attn_f16_v0<false>, grid, dim3(256), 0, s, qkv, out, L, Lq, H, nT, nWG, attn::SCALE_LOG2E);
    return (int)hipGetLastError();
}

int launch_attention_f32(const float* qkv, float* out, const AggSeqs& q, int H, int max_len, hipStream_t s) {
    if (q.nseq <= 0 || q.M <= 0) return 0;
    switch (route_f32(q.len, max_len)) {
    case F32_REFUSED: return -2;
    case F32_SMALL: {
        const size_t lds = (size_t)2 * q.len * 64 * sizeof(float);
        const dim3 grid((unsigned)q.nseq * H);
        if (q.offsets) hipLaunchKernelGGL(attn_f32_small<true>, grid, dim3(128), lds, s, qkv, out, q, H, 0.125f);
        else hipLaunchKernelGGL(attn_f32_small<false>, grid, dim3(128), lds, s, qkv, out, q, H, 0.125f);
        return (int)hipGetLastError();
    }
    case F32_LONG: break;
    }
    return launch_attention_f32_long(qkv, out, q, H, s);
}

// attn_f32_long at any q.len up to the ceiling (the generator comes here through launch_attention_f32; ovmr_debug_attention_f32_long
// directly, short launches included).  One workgroup per (sequence, head, 128-row query tile of the LONGEST sequence): the tiles of a
// shorter one that start behind its end leave at once, so a 500-row class among a thousand short ones adds its own four tiles per
// head and three empty ones per other (class, head), and nothing waits for it.
int launch_attention_f32_long(const float* qkv, float* out, const AggSeqs& q, int H, hipStream_t s) {
    if (q.nseq <= 0 || q.M <= 0) return 0;
    if (q.len < 1 || q.len > OVMR_AGG_MAX_LEN_CEILING) return -2;
    const int nT = (q.len + attn::F32_TILE - 1) / attn::F32_TILE;
    const long wgs = (long)q.nseq * H * nT;
    if (wgs > 0x7fffffffL) return -2;
    const dim3 grid((unsigned)wgs), block(attn::F32_TILE);
    if (q.offsets) hipLaunchKernelGGL(attn_f32_long<true>, grid, block, 0, s, qkv, out, q, H, nT, 0.125f);
    else hipLaunchKernelGGL(attn_f32_long<false>, grid, block, 0, s, qkv, out, q, H, nT, 0.125f);
    return (int)hipGetLastError();
}
