// The launch plan of the fp16 GEMM family.  gemm_f16_route (gemm_f16.hip) is the ONE place that decides which kernel a launch runs
// and with which compile-time options; the launchers of gemm_f16.hip, gemm_f16_small.hip and gemm_f16_v5.hip run the plan they are
// handed and return -3 for one they hold no kernel for.  Every kernel computes the same values, so a mistake in the route costs time,
// not correctness: tests/test_gemm_route_cpu.py holds it to a restatement in Python (ovmr_debug_gemm_route, no GPU).
#pragma once
#include "common.h"

enum GemmKernel {
    GEMM_NONE = 0,   // nothing is launched: launch_gemm_f16 returns GemmPlan::rc (0: empty shape)
    GEMM_T128 = 1,   // gemm_f16.hip: 128 x 128 register-staged tiles, every shape
    GEMM_S64 = 2,    // gemm_f16_small.hip: 64 x 64 tiles, K split over the waves
    GEMM_TILE = 3,   // gemm_f16_v5.hip: 256(128) x 256 LDS-DMA tiles, fused epilogues
};
enum GemmLoop { LOOP_DOUBLE = 0, LOOP_BOUNDARY = 1, LOOP_PINGPONG = 2 };   // K loops of the tile kernel (gemm_f16_v5.hip)

struct GemmPlan {
    int kernel, rc;
    int depth, groups;                                // GEMM_S64: K-steps of 32 prefetched per wave, K groups of `depth` steps per wave
    int tile_rows, loop, a_nt, nt_store, n_group;     // GEMM_TILE: 128 / 256, GemmLoop, nontemporal A stream / C stores, GemmArgs::n_group
    int gelu_mode;                                    // GemmArgs::gelu_mode of the launch (0 unless the epilogue is a QuickGELU one)
    int persist;                                      // GEMM_TILE, LayerNorm-fold ping-pong launches: one workgroup per CU walks the tiles (gemm_f16_v5.hip, "Tile loop")
};
GemmPlan gemm_f16_route(const GemmArgs& a, int variant);
int launch_gemm_f16_small(const GemmArgs& a, const GemmPlan& p, hipStream_t s);
int launch_gemm_f16_v5(const GemmArgs& a, const GemmPlan& p, hipStream_t s, int max_wgs = 0);   // max_wgs > 0: caps a persistent grid (tests)
// For the engine: does `variant` send an [M, N] launch to the split-K kernel because the shape is latency-bound (K permitting), and
// the variant that pins, for a launch on PART of an [M, N] problem, the kernel family the whole launch takes under `variant`.
bool gemm_f16_latency_bound(int variant, int M, int N);
int gemm_f16_pinned_variant(int variant, int M, int N);
