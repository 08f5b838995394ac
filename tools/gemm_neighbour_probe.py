#!/usr/bin/env python3
"""Does an unchanged kernel run slower behind the tile-loop form of c_fc than behind its one-workgroup-per-tile form?  c_fc (ln_2 fold +
one-rounding QuickGELU, M = 775 x 197) and c_proj (<3, 8, 17>) are launched alternately, twelve pairs per block with HIP events around every
launch, blocks with gemm_persist 0 and 1 alternating in one process; prints us per launch of either kernel per block (the last ten pairs).

    python tools/gemm_neighbour_probe.py
"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ovmr_amd import runtime
lib = runtime.load_library()
c_i, c_p = ctypes.c_int, ctypes.c_void_p
lib.ovmr_debug_gemm_persist.restype = c_i
lib.ovmr_debug_gemm_persist.argtypes = [c_i, c_p, c_i, c_p, c_p, c_p, c_i, c_i, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p]
p = lambda t: ctypes.c_void_p(t.data_ptr())
s = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
M, D = 775 * 197, 768
g = torch.Generator(device="cuda").manual_seed(1)
x = (torch.randn((M + 256, D), generator=g, device="cuda") * 0.5).half()
Wfc = (torch.randn((4 * D + 256, D), generator=g, device="cuda") * D ** -0.5).half()
Wpj = (torch.randn((D + 256, 4 * D), generator=g, device="cuda") * (4 * D) ** -0.5).half()
b = (torch.randn((D,), generator=g, device="cuda") * 0.1).half()
hid = torch.zeros((M, 4 * D), dtype=torch.float16, device="cuda")
st = torch.zeros((M, 3, 2), device="cuda"); st[:, 0, 1] = float(D)
lg, lb = torch.ones(4 * D, device="cuda"), torch.zeros(4 * D, device="cuda")
so = torch.zeros((M, 3, 2), device="cuda")
xo = x[:M].clone()
def fc(ps): assert lib.ovmr_debug_gemm_persist(108, p(x), D, p(Wfc), p(lb), p(st), 3, 0, p(lg), p(hid), 4 * D, M, 4 * D, D, 7, ps, 0, s()) == 0
def pj(): assert lib.ovmr_debug_gemm(0, 8, p(hid), p(Wpj), p(b), p(xo), p(so), p(xo), M, D, 4 * D, D, 3, 1.0, 0, 0, s()) == 0
for ps in (0, 1): fc(ps); pj()
torch.cuda.synchronize()
res = {0: ([], []), 1: ([], [])}
for rnd in range(6):
    for ps in (0, 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3 * 12)]
        for i in range(12):
            ev[3 * i].record(); fc(ps); ev[3 * i + 1].record(); pj(); ev[3 * i + 2].record()
        torch.cuda.synchronize()
        res[ps][0].append(sum(ev[3 * i].elapsed_time(ev[3 * i + 1]) for i in range(2, 12)) * 100)
        res[ps][1].append(sum(ev[3 * i + 1].elapsed_time(ev[3 * i + 2]) for i in range(2, 12)) * 100)
for ps in (0, 1):
    print(f"gemm_persist {ps}: c_fc us per launch {[round(t, 1) for t in res[ps][0]]}  c_proj behind it {[round(t, 1) for t in res[ps][1]]}  pair {[round(a + b, 1) for a, b in zip(*res[ps])]}")
