// What the fp16 attention kernels (hd = 64) share: the launchers behind launch_attention_f16_q with the shapes each one takes,
// and one definition of every step that more than one kernel uses.  Lane naming of the 16x16x32 kernels: fr = lane & 15 is the
// query row of the tile, fg = lane >> 4 the key quartet (S^T = K Q^T puts the keys on the accumulator rows).
#pragma once
#include "common.h"

namespace attn {

// ---- the kernels and their shapes ---------------------------------------------------------------------------------------------
// route() in attention.hip is the one place that picks a kernel; a launcher handed another shape returns OVMR_E_SHAPE.
// attention.hip, attn_f16_v0: every shape.
// attention_short.hip, attn_f16_short (launch_attention_f16_short, common.h): whole sequences of at most 32 tokens.
inline bool short_takes(int L, int Lq) { return Lq == L && L <= 32; }
// attention_v1.hip: every shape; route() sends it L >= 128 (below that there is one key block or two and variant 0 is faster,
// tools/attn_bench.py).
int launch_attention_f16_v1(const half_t* qkv, half_t* out, int B, int L, int Lq, int H, int causal, hipStream_t s);
inline bool v1_wanted(int L) { return L >= 128; }
// attention_v3.hip: the ViT-B/16 image shape, all 13 key sub-tiles of a head in LDS at once.  -100: the device index is outside the
// launcher's per-device table (the caller runs variant 1).
int launch_attention_f16_v3(const half_t* qkv, half_t* out, int B, int L, int H, hipStream_t s);
inline bool v3_takes(int L, int Lq, int causal) { return !causal && Lq == L && L > 192 && L <= 208; }
// attention_v5.hip: no mask, at least four key blocks and one 32-row query tile (ViT-L: L = 257 / 577).
int launch_attention_f16_v5(const half_t* qkv, half_t* out, int B, int L, int Lq, int H, hipStream_t s);
inline bool v5_takes(int L, int Lq, int causal) { return !causal && L >= 256 && Lq >= 32; }

constexpr float SCALE_LOG2E = 0.125f * 1.4426950408889634f;   // hd^-0.5 * log2(e), hd = 64: p = exp2(s * SCALE_LOG2E - m)

// XCD placement (variants 1 and 5): workgroups are dealt to the 8 XCDs by block id mod 8, so the nWG workgroups of one (sequence,
// head) bh get block ids congruent mod 8 -- one XCD, whose L2 then serves their K / V re-reads.  The grid is rounded up to whole
// rounds of 8 heads; the decode's bh may therefore be >= nBH (such a workgroup returns).
struct Placement { int wg, bh; };
inline unsigned xcd_grid(int nBH, int nWG) { return (unsigned)((long)((nBH + 7) / 8) * 8 * nWG); }
__device__ __forceinline__ Placement xcd_decode(unsigned block, int nWG) {
    const int xcd = block & 7, slot = block >> 3;
    return {slot % nWG, (slot / nWG) * 8 + xcd};
}

// ---- LDS-DMA and the transposing read -----------------------------------------------------------------------------------------
typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;
typedef short short4v __attribute__((__vector_size__(8)));

// LDS-DMA (global_load_lds_dwordx4: 16 bytes per lane, the wave's 1 KiB piece at LDS byte address M0) issued from inline asm, with M0
// saved and restored inside the statement, so that hipcc does not know an LDS write is in flight.  With the builtin it puts an
// `s_waitcnt vmcnt(0)` in front of the first transposing V read after the issue -- in variant 3 that waits for the NEXT head's whole
// K / V stream before the PV products, in variant 5 it drains the blocks in flight in every key block: the overlap both kernels
// exist for.  Ordering is the CALLER's, by hand: a counted wait and a workgroup barrier at the top of its head / block loop.
// (Waits hipcc computes for its own loads ignore these DMAs and can therefore only be too strict.)
// Two address forms: a 64-bit global address per lane ...
__device__ __forceinline__ void glds16_asm(const void* gsrc, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
// ... and a scalar base + 32-bit per-lane byte offset: a walk over key blocks is one scalar add, the per-lane offsets never change.
__device__ __forceinline__ void glds16_asm(const void* sbase, unsigned voff, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}

// ds_read_b64_tr_b16: per 16-lane group the instruction reads 4 keys x 16 d of a row-major [key][d] image and hands lane i the
// 4 keys of column d0 + i -- a V^T fragment (A operand of O^T = V^T P^T) without a transposing store.
__device__ __forceinline__ half4_t tr_read(const half_t* p) {
    short4v r = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)p);
    return __builtin_bit_cast(half4_t, r);
}

// Where lane (fr, fg) points its transposing read in a V image of 128-byte rows with chunk c of row r in slot c ^ (r & 7) (variants
// 1 and 3), in halves: for the 16 keys from k0 on, key row kr = vt_row(k0, fr, fg) at kr * 64, and in that row, for d tile dt, 4 d
// columns at vt_col(kr, dt, fr).  The fragment's second half, keys + 16, has the same column offset: (kr + 16) & 7 == kr & 7.
__device__ __forceinline__ int vt_row(int k0, int fr, int fg) { return k0 + fg * 4 + (fr >> 2); }
__device__ __forceinline__ int vt_col(int kr, int dt, int fr) {
    const int c = dt * 2 + ((fr & 3) >> 1);
    return ((c ^ (kr & 7)) << 3) + (fr & 1) * 4;
}

// ---- across the lanes of a query --------------------------------------------------------------------------------------------
// x of this lane and of lane l ^ 32, in the order (lower half's, upper half's) on both: v_permlane32_swap exchanges the 32-lane
// halves between two registers, and with both operands = x the two results are those two values.  No LDS crossbar (ds_bpermute
// is a ~100-cycle LDS round trip in the max -> exp dependency chain).  Variant 5 keeps a query in lanes l and l + 32.
__device__ __forceinline__ float2_t pair32(float x) {
    const unsigned u = __builtin_bit_cast(unsigned, x);
    auto sw = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return (float2_t){__builtin_bit_cast(float, (unsigned)sw[0]), __builtin_bit_cast(float, (unsigned)sw[1])};
}

// max over the four lanes {l, l^16, l^32, l^48} that hold one query row's scores in the 16x16x32 kernels: the same exchange with
// v_permlane16_swap, then pair32.
__device__ __forceinline__ float row_max4(float x) {
    const unsigned u = __builtin_bit_cast(unsigned, x);
    auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    const float2_t p = pair32(fmaxf(__builtin_bit_cast(float, (unsigned)a[0]), __builtin_bit_cast(float, (unsigned)a[1])));
    return fmaxf(p[0], p[1]);
}

// ---- softmax steps --------------------------------------------------------------------------------------------------------
// The LAZY reference maximum of variants 1 and 5.  m_run is the maximum the exponentials are taken against (scaled domain).  It
// only moves when some row's block maximum mxs exceeds it by more than LAZY_THRESHOLD = 8: a factor 256 in p, harmless for fp16 P
// (p <= 2^8) and fp32 accumulators.  Then rescale(alpha) multiplies the caller's accumulators and row sums by alpha =
// exp2(m_old - m_new).  After the first key block that is rare, so the packed multiplies and the exponential of the usual
// every-block rescale disappear (variant 1 is bound by the VALU issue port, profiles/r01g_pmc_attn.json).  The test is a ballot:
// wave-uniform, and a reference stays stale only while no row of the wave asks for a move (tests/attn_exact.py, three_level).
constexpr float LAZY_THRESHOLD = 8.0f;
template <class Rescale>
__device__ __forceinline__ void lazy_reference(float mxs, float& m_run, Rescale rescale) {
    if (__builtin_amdgcn_ballot_w64(mxs > m_run + LAZY_THRESHOLD) != 0) {
        const float m_new = fmaxf(m_run, mxs);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);   // raw v_exp_f32: the argument is <= 0 (first block: -inf -> 0)
        m_run = m_new;
        rescale(alpha);
    }
}

// The exponential half of the EXACT softmax step of attn_f16_v0 (NT = 4 key sub-tiles of 16 per block) and attn_f16_short (NT = 2):
// lane (fr, fg) holds the masked, scaled scores of its query against the keys nt * 16 + fg * 4 + r of the block.  p = exp2(s - m) in
// place, against the maximum m the caller settled on (variant 0: the running one, the short kernel: the row's); returns the row
// sum, fp32, by two shuffles.  Both kernels go through this one function: their sums add in the same order.
template <int NT>
__device__ __forceinline__ float exp_sum(float4_t (&s)[NT], float m) {
    float psum = 0.f;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float p = exp2f(s[nt][r] - m);
            s[nt][r] = p;
            psum += p;
        }
    psum += __shfl_xor(psum, 16, 64);
    return psum + __shfl_xor(psum, 32, 64);
}

// ---- epilogue -------------------------------------------------------------------------------------------------------------
// Normalise and store this lane's 16 outputs of one query row: o[dt] holds d = dt * 16 + fg * 4 + [0, 4), op points at the row's
// d = fg * 4.
__device__ __forceinline__ void store_row4(half_t* op, const float4_t (&o)[4], float inv) {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        const half4_t w = {(half_t)(o[dt][0] * inv), (half_t)(o[dt][1] * inv), (half_t)(o[dt][2] * inv), (half_t)(o[dt][3] * inv)};
        *(half4_t*)(op + dt * 16) = w;
    }
}

// ---- the fp32 kernels (attention.hip: attn_f32_small and attn_f32_long, both modes of each) -------------------------------------
// One query row against the keys of its own (sequence, head), K and V of a key block in LDS as [key][64] fp32: keys in increasing
// order, s summed over d in increasing order and then scaled, the online maximum, __expf, l and o updated in this order, one
// reciprocal at the end.  The row is three steps over one state -- begin, keys (once per staged block, the blocks in key order), end
// -- and every kernel goes through these three functions.  The library is built with -ffp-contract=off and without fast-math, so a row
// walked over its keys 0 .. L - 1 gives the same bits whether the keys were staged in one block or in several: a row's bits do not
// depend on which kernel ran it, on L of any other sequence, or on where the row sits in the launch.
struct F32Row {
    float qv[64], o[64], m, l;
};
__device__ __forceinline__ void f32_row_begin(F32Row& r, const float* __restrict__ qrow) {
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        float4_t t = *(const float4_t*)(qrow + c * 4);
        r.qv[c * 4] = t[0]; r.qv[c * 4 + 1] = t[1]; r.qv[c * 4 + 2] = t[2]; r.qv[c * 4 + 3] = t[3];
    }
#pragma unroll
    for (int d = 0; d < 64; ++d) r.o[d] = 0.f;
    r.m = -INFINITY;
    r.l = 0.f;
}
// the keys [k0, k1) of the block staged at sK / sV (m and l in locals over the loop: attn_f32_small then compiles to the
// instructions it had when the row was one function)
__device__ __forceinline__ void f32_row_keys(F32Row& r, const float* sK, const float* sV, int k0, int k1, float scale) {
    float m = r.m, l = r.l;
    for (int key = k0; key < k1; ++key) {
        float s = 0.f;
#pragma unroll
        for (int d = 0; d < 64; ++d) s += r.qv[d] * sK[key * 64 + d];
        s *= scale;
        const float mn = fmaxf(m, s);
        const float alpha = __expf(m - mn), p = __expf(s - mn);
        l = l * alpha + p;
#pragma unroll
        for (int d = 0; d < 64; ++d) r.o[d] = r.o[d] * alpha + p * sV[key * 64 + d];
        m = mn;
    }
    r.m = m;
    r.l = l;
}
__device__ __forceinline__ void f32_row_end(const F32Row& r, float* __restrict__ orow) {
    const float inv = 1.0f / r.l;
#pragma unroll
    for (int c = 0; c < 16; ++c)
        *(float4_t*)(orow + c * 4) = (float4_t){r.o[c * 4] * inv, r.o[c * 4 + 1] * inv, r.o[c * 4 + 2] * inv, r.o[c * 4 + 3] * inv};
}

// The shapes of the two kernels.  attn_f32_small holds a whole sequence's K and V in LDS: 128 rows are its 64 KiB.  attn_f32_long takes
// 128 query rows per workgroup (a thread each) and stages 64 keys per block, 32 KiB: with a thousand short classes beside one long one
// most workgroups of a launch are short or leave at once, and at 64 KiB two of them fill a CU's LDS (measured with 128-key blocks:
// 10.8 against 8.7 ms).  The block size changes no bit: the keys are walked in the same order.
constexpr int F32_SMALL_MAX = 128, F32_TILE = 128, F32_KEYS = 64;

}  // namespace attn
