"""What exemplar classes beyond 126 images need away from the GPU: the exact-operand builder accepts the lengths
tests/test_hip_agg_long_kernels.py launches (a change to the builder cannot silently empty that test), the runner refuses a uniform
NUM_SHOTS larger than a loader batch in one line, and CustomCLIP refuses more aggregator rows per class than the engine takes, by name.
"""
import os

import pytest
import torch

import agg_long_cases as C
import attn_exact as A
from conftest import REPO


def test_gpu_test_covers_the_block_and_tile_edges():
    assert C.EXACT_L == (129, 130, 255, 256, 257, 385, 513) and C.EXACT_UNIFORM_L == (256, 512)
    assert len(C.EXACT) == 16 and sorted(C.MIXED) == ["eight_heads", "two_heads"]


@pytest.mark.parametrize("L", C.EXACT_L)
@pytest.mark.parametrize("kind", ["onehot", "groups"])
def test_builder_accepts_long_fp32_lengths(kind, L):
    """The builder's own assertions (code distance, distinct V rows, power-of-two group sizes, fp32-exact expectations) hold, every
    row is finite, and the expected rows are what the fp64 softmax gives on the same operands to 1e-6."""
    built = A.build(kind, L, True)
    assert built.qkv.shape == (A.B * L, 3 * A.H * 64) and built.want.shape == (A.B * L, A.H * 64)
    assert built.qkv.dtype == built.want.dtype == torch.float32 and bool(torch.isfinite(built.want).all())
    q, k, v = built.qkv.double().reshape(A.B, L, 3, A.H, 64).permute(2, 0, 3, 1, 4)
    ref = ((q @ k.transpose(-1, -2) * 0.125).softmax(-1) @ v).permute(0, 2, 1, 3).reshape(A.B * L, A.H * 64)
    assert float((built.want.double() - ref).abs().max()) < 1e-6


@pytest.mark.parametrize("L", C.EXACT_UNIFORM_L)
def test_builder_accepts_long_fp32_uniform_lengths(L):
    built = A.build("uniform", L, True)
    assert built.want.shape == (A.B * L, A.H * 64) and bool((built.qkv[:, :A.H * 64] == 0).all())
    v = built.qkv.double().reshape(A.B, L, 3, A.H, 64)[:, :, 2]
    assert torch.equal(built.want.double().reshape(A.B, L, A.H, 64), v.mean(1, keepdim=True).expand(-1, L, -1, -1))


def test_runner_refuses_uniform_shots_above_the_loader_batch(monkeypatch, tmp_path):
    from ovmr_amd import checkpoint, cli, runtime

    def boom(*a, **k):
        raise AssertionError("the runner touched the model / library before refusing the job")

    monkeypatch.setattr(runtime, "load_library", boom)
    monkeypatch.setattr(checkpoint, "load_clip_state_dict", boom)
    argv = ["--root", str(tmp_path / "nowhere"), "--trainer", "MM_CLS_OP", "--eval-only", "--clip-weights", str(tmp_path / "none.pt"),
            "--output-dir", str(tmp_path / "out"), "DATASET.NUM_SHOTS", "512", "DATALOADER.TEST.BATCH_SIZE", "256"]
    with pytest.raises(SystemExit, match=r"TEST\.BATCH_SIZE 256 is smaller than DATASET\.NUM_SHOTS 512.*whole classes.*raise TEST\.BATCH_SIZE") as e:
        cli.main(argv)
    assert "\n" not in str(e.value)
    assert not (tmp_path / "out").exists()


def test_custom_clip_refuses_more_rows_than_the_engine_takes():
    """n_ctx + NUM_SHOTS above 4096 (NUM_SHOTS above 4094 at n_ctx = 2): a ValueError that names the key, before any engine exists."""
    from ovmr_amd import modules
    assert modules.AGG_MAX_LEN_CEILING == 4096
    header = open(os.path.join(REPO, "include", "ovmr_hip.h")).read()
    assert "#define OVMR_AGG_MAX_LEN_CEILING 4096" in header
    cfg = modules.make_cfg(n_ctx=2, num_shots=4095, output_dir="", test_batch_size=4095)
    with pytest.raises(ValueError, match="DATASET.NUM_SHOTS 4095"):
        modules.CustomCLIP(cfg, torch.zeros(1, 77, dtype=torch.int64), None)
