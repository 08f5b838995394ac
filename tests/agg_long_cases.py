"""The case tables of tests/test_hip_agg_long_kernels.py (GPU), shared with tests/test_agg_long_cpu.py, which holds attn_exact's builder
to them on the CPU.  No library, no GPU."""

# attn_f32_long takes 128 query rows per tile and stages 64 keys per block (every multiple of 128 is a block edge too): one row past a
# tile, two, one short of two tiles, two tiles, one more, three tiles + 1, four + 1.  attn_exact's fp32 uniform case needs a
# power-of-two length.
EXACT_L, EXACT_UNIFORM_L = (129, 130, 255, 256, 257, 385, 513), (256, 512)
EXACT = [(k, L) for L in EXACT_L for k in ("onehot", "groups")] + [("uniform", L) for L in EXACT_UNIFORM_L]

# (H, lengths, n_ctx) of the mixed table launches: a sequence of length n is n_ctx context rows + (n - n_ctx) shots
MIXED = {
    "two_heads": (2, [1, 5, 128, 129, 64, 300, 2, 257, 127], 0),
    "eight_heads": (8, [3, 130, 66], 2),
}
