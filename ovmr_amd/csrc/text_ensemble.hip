// Prompt ensembling of ZeroshotCLIP2.build_model (trainers/zsclip.py:88-96): the per-template text features of a chunk of classes
// -> one normalised classifier row per class.  The text tower itself runs in ovmr_api.hip (ovmr_encode_text_ensemble: all templates of
// the chunk as the groups of ONE tower pass, raw projected rows into a [T, rows, E] scratch of the workspace); this launch does the rest.
//
// The fp16 rounding points of the reference's GPU path (fp16 model, every tensor op rounds its result to fp16):
//   n_t = h(||x_t||)            squares accumulated in fp32 (x.norm() on an fp16 tensor; l2norm_f16_kernel in rowops.hip)
//   u_t = h(x_t / n_t)          :92-93
//   acc = u_0, acc = h(acc + u_t) for t = 1 ... T-1, in template order (:94; `0 + u_0` is u_0)
//   m   = h(acc * (1 / T))      :95 -- an fp16 tensor divided by a host scalar runs as a multiplication by the fp32 reciprocal in
//                               PyTorch's GPU kernel (div_true with a CPU-scalar divisor), so that is the rounding kept here
//   out = h(m / h(||m||))       :96
// One wave per class row; the wave keeps the row's running sum in registers and reads each template's row exactly once.
#include "common.h"

namespace {

// 16-byte path: E % 8 == 0, 16-byte aligned rows, E <= 512 * NCH.  Lane l holds columns 8 l + 512 j ... + 7 of the row, j < NCH.
template <int NCH>
__global__ __launch_bounds__(256) void text_ensemble_v8_kernel(const half_t* __restrict__ feats, int T, int rows, int E, float inv_T,
                                                               half_t* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    half8_t acc[NCH];
    for (int t = 0; t < T; ++t) {
        const half_t* xr = feats + ((long)t * rows + row) * E;
        half8_t x[NCH];
        float ss = 0.f;
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const int c = lane * 8 + j * 512;
            if (c < E) {
                x[j] = *(const half8_t*)(xr + c);
#pragma unroll
                for (int k = 0; k < 8; ++k) ss += (float)x[j][k] * (float)x[j][k];
            }
        }
        const float n = fmaxf((float)(half_t)sqrtf(wave_sum(ss)), 1e-12f);
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            if (lane * 8 + j * 512 < E) {
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const half_t u = (half_t)((float)x[j][k] / n);
                    acc[j][k] = t == 0 ? u : (half_t)((float)acc[j][k] + (float)u);
                }
            }
        }
    }
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        if (lane * 8 + j * 512 < E) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                acc[j][k] = (half_t)((float)acc[j][k] * inv_T);
                ss += (float)acc[j][k] * (float)acc[j][k];
            }
        }
    }
    const float n = fmaxf((float)(half_t)sqrtf(wave_sum(ss)), 1e-12f);
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int c = lane * 8 + j * 512;
        if (c < E) {
            half8_t o;
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k] = (half_t)((float)acc[j][k] / n);
            *(half8_t*)(out + (long)row * E + c) = o;
        }
    }
}

// Any E, any alignment: element by element, the running sum kept in the output row itself (it is an fp16 value at every step).
__global__ __launch_bounds__(256) void text_ensemble_any_kernel(const half_t* __restrict__ feats, int T, int rows, int E, float inv_T,
                                                                half_t* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    half_t* o = out + (long)row * E;
    for (int t = 0; t < T; ++t) {
        const half_t* xr = feats + ((long)t * rows + row) * E;
        float ss = 0.f;
        for (int c = lane; c < E; c += 64) ss += (float)xr[c] * (float)xr[c];
        const float n = fmaxf((float)(half_t)sqrtf(wave_sum(ss)), 1e-12f);
        for (int c = lane; c < E; c += 64) {
            const half_t u = (half_t)((float)xr[c] / n);
            o[c] = t == 0 ? u : (half_t)((float)o[c] + (float)u);
        }
    }
    float ss = 0.f;
    for (int c = lane; c < E; c += 64) {
        const half_t m = (half_t)((float)o[c] * inv_T);
        o[c] = m;
        ss += (float)m * (float)m;
    }
    const float n = fmaxf((float)(half_t)sqrtf(wave_sum(ss)), 1e-12f);
    for (int c = lane; c < E; c += 64) o[c] = (half_t)((float)o[c] / n);
}

}  // namespace

// feats: [T, rows, E] fp16 (template-major), out: [rows, E] fp16; out must not overlap feats.
int launch_text_ensemble(const half_t* feats, int T, int rows, int E, half_t* out, hipStream_t s) {
    if (rows <= 0) return 0;
    const dim3 grid((rows + 3) / 4), block(256);
    const float inv_T = 1.0f / (float)T;
    const bool v8 = E % 8 == 0 && ((uintptr_t)feats & 15) == 0 && ((uintptr_t)out & 15) == 0;
    if (v8 && E <= 512) hipLaunchKernelGGL(text_ensemble_v8_kernel<1>, grid, block, 0, s, feats, T, rows, E, inv_T, out);
    else if (v8 && E <= 1024) hipLaunchKernelGGL(text_ensemble_v8_kernel<2>, grid, block, 0, s, feats, T, rows, E, inv_T, out);
    else hipLaunchKernelGGL(text_ensemble_any_kernel, grid, block, 0, s, feats, T, rows, E, inv_T, out);
    return (int)hipGetLastError();
}
