"""Worker of tests/test_hip_ragged.py: one rank of a multi-process RAGGED classifier-generation job on the real engine (24 classes,
shots cycling through 1, 3, 8, 16; several ranks share the test box's one GPU over gloo, as tests/dist_gpu_worker.py does for the
uniform job).

    RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT in the environment;  argv: <result path>"""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ovmr_amd import modules, synth  # noqa: E402
from ovmr_amd.data import ResidentRaggedSet  # noqa: E402

SEED, C, CYCLE = 11, 24, (1, 3, 8, 16)


def main():
    result = sys.argv[1]
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    spec = synth.SPECS["small"]
    sd = {k: torch.from_numpy(v) for k, v in synth.clip_state_dict(spec, SEED, jitter=True).items()}
    pl = {k: torch.from_numpy(v) for k, v in synth.prompt_learner_state_dict(spec, 2, SEED, True).items()}
    cm = modules.CLIPModel(sd, spec, "cuda:0")
    out_dir = os.path.join(os.path.dirname(result), f"out_w{world}")
    cfg = modules.make_cfg(n_ctx=2, num_shots=16, output_dir=out_dir, test_batch_size=40)
    tok = torch.from_numpy(synth.class_token_ids(C, seed=4321))
    model = modules.CustomCLIP(cfg, tok, cm, prompt_learner_state=pl, reserve=(64, 64, 64))
    shots = [CYCLE[c % len(CYCLE)] for c in range(C)]
    labels = np.repeat(np.arange(C), shots)
    img = torch.from_numpy(synth.images(len(labels), spec.image_resolution, 1234, labels, 0.6)).cuda().half()
    loader = ResidentRaggedSet(img, labels, 40, rank, world, C)
    model.forward_prompt(loader)              # (both files are on disk when it returns)
    torch.cuda.synchronize()
    if rank == 0:
        files = {f: torch.load(os.path.join(out_dir, f), map_location="cpu") for f in sorted(os.listdir(out_dir))}
        torch.save({"mm": model.mm_classifier.cpu(), "v": model.visual_classifer.cpu(), "t": model.zero_shot_classifier.cpu(),
                    "w": model.fusion_weight.cpu(), "counts": model.xval_counts.cpu(), "tokens": model.visual_tokens.cpu(),
                    "classes": sorted(set(labels.tolist())), "files": files, "sharded_path": model._dist is not None,
                    "local_rows": int(model.eval_feat4cls.shape[0])}, result)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
