#!/usr/bin/env python3
"""Generate tests/golden/zsclip.npz by running the REAL zero-shot trainers of the reference (trainers/zsclip.py).

Runs ONLY in the build container (needs the reference checkout, which never travels to the GPU box).  It reuses gen_golden.py's harness
(name-only stubs for torchvision / ftfy / torcheval / dassl, .cuda() as the identity) and adds one stub: `trainers.coop`, whose
`load_clip_to_cpu` returns the seeded synthetic ViT-B/16 of ovmr_amd/synth.py (seed 11, fp16 as build_model leaves it, or after
`.float()`).  dassl.engine's TRAINER_REGISTRY.register() returns the class unchanged, so `ZeroshotCLIP.build_model` /
`ZeroshotCLIP2.build_model` / `model_inference` run as written, on objects made without TrainerX's constructor (cfg, dm and device set by
hand).  The reference appends the dataset's template to the CLASS attribute of ZeroshotCLIP2 (:83); the list is restored after every
build so that each build sees the reference's first-build template count.

Recorded (no reference source, bytecode or vocabulary is copied; only inputs that cannot be regenerated and the reference's outputs):
  zs_classnames, zs_templates_<dataset> (Caltech101: 8, ImageNet: 7), zs_dataset_templates (name -> template, as two arrays),
  zs_token_ids [8, 10, 77] (the real clip.tokenize, template-major; ImageNet's 7 are the first 7), merge_ranks / merge_pairs (the merges of
  the reference's BPE table these prompts reach, in bpe_merges.npz's form), and per trainer zsclip / zsclip2 and model tag fp16 / fp32:
  <trainer>_<tag>_text_features [10, 512] and <trainer>_<tag>_logits [16, 10] on synth.images(16, 224, seed=1234); for ZeroshotCLIP2
  also on ImageNet's 7 templates (zsclip2_imagenet_<tag>_text_features).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_zsclip.py
"""
from __future__ import annotations

import os
import sys
import types
from types import SimpleNamespace

sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: E402
from gen_golden import REF, build_ref_clip  # noqa: E402
from ovmr_amd import synth  # noqa: E402

# ten Caltech-101 categories (the CoOp split's folder names), several with underscores
CLASSNAMES = ["accordion", "airplane", "crocodile_head", "dollar_bill", "grand_piano", "sea_horse", "stop_sign", "water_lilly",
              "wild_cat", "yin_yang"]
ZS = dict(spec="ViT-B/16", seed=11, n_img=16, img_seed=1234)


def import_zsclip():
    ref_model, ref_clip, _ = gen_golden.import_reference()
    state = {"fp32": False}

    def load_clip_to_cpu(cfg):
        return build_ref_clip(ref_model, synth.SPECS[ZS["spec"]], ZS["seed"], True, state["fp32"])

    import trainers                                                        # the reference's (empty) package
    coop = types.ModuleType("trainers.coop")
    coop.load_clip_to_cpu = load_clip_to_cpu
    sys.modules["trainers.coop"] = coop
    trainers.coop = coop
    import trainers.zsclip as zs
    return ref_clip, zs, state


def build(zs, cls, dataset):
    t = object.__new__(cls)
    t.cfg = SimpleNamespace(DATASET=SimpleNamespace(NAME=dataset), MODEL=SimpleNamespace(BACKBONE=SimpleNamespace(NAME=ZS["spec"])))
    t.dm = SimpleNamespace(dataset=SimpleNamespace(classnames=list(CLASSNAMES)))
    t.device = "cpu"
    saved = list(zs.ZeroshotCLIP2.templates)
    try:
        with torch.no_grad():
            t.build_model()
    finally:
        zs.ZeroshotCLIP2.templates[:] = saved                             # undo :83 (the class attribute grows on every build)
    return t


def merges_reached(texts, out):
    """gen_golden.gen_bpe_merges for `texts`: the merges of the reference's table BPE looks up while it tokenises them, with their ranks."""
    from ovmr_amd.tokenizer import BPETokenizer
    tk = BPETokenizer(os.path.join(REF, "clip", "bpe_simple_vocab_16e6.txt.gz"))
    seen = {}

    class Probe(dict):
        def get(self, key, default=None):
            r = dict.get(self, key, default)
            if r is not None:
                seen[key] = r
            return r

    tk.rank = Probe(tk.rank)
    tk.tokenize(texts)
    pairs = sorted(seen, key=seen.get)
    out["merge_ranks"] = np.array([seen[p] for p in pairs], dtype=np.int64)
    out["merge_pairs"] = np.array([" ".join(p) for p in pairs])


def main():
    torch.set_num_threads(os.cpu_count())
    ref_clip, zs, state = import_zsclip()
    out = {"zs_classnames": np.array(CLASSNAMES)}
    names = sorted(zs.CUSTOM_TEMPLATES)
    out["zs_dataset_names"] = np.array(names)
    out["zs_dataset_templates"] = np.array([zs.CUSTOM_TEMPLATES[n] for n in names])
    temps = {"Caltech101": list(zs.ZeroshotCLIP2.templates) + [zs.CUSTOM_TEMPLATES["Caltech101"]],      # :68, :82-83
             "ImageNet": list(zs.ZeroshotCLIP2.templates)}
    for ds, ts in temps.items():
        out[f"zs_templates_{ds}"] = np.array(ts)
    texts = [[t.format(c.replace("_", " ")) for c in CLASSNAMES] for t in temps["Caltech101"]]          # :43, :90
    out["zs_prompts"] = np.array(texts)
    out["zs_token_ids"] = torch.stack([torch.cat([ref_clip.tokenize(p) for p in ps]) for ps in texts]).numpy()   # :45, :91
    merges_reached([p for ps in texts for p in ps], out)
    img = torch.from_numpy(synth.images(ZS["n_img"], synth.SPECS[ZS["spec"]].image_resolution, seed=ZS["img_seed"]))
    for tag, fp32 in (("fp16", False), ("fp32", True)):
        state["fp32"] = fp32
        for key, cls, ds in (("zsclip", zs.ZeroshotCLIP, "Caltech101"), ("zsclip2", zs.ZeroshotCLIP2, "Caltech101"),
                             ("zsclip2_imagenet", zs.ZeroshotCLIP2, "ImageNet")):
            t = build(zs, cls, ds)
            out[f"{key}_{tag}_text_features"] = t.text_features.float().numpy()
            if key != "zsclip2_imagenet":
                with torch.no_grad():
                    out[f"{key}_{tag}_logits"] = t.model_inference(img).float().numpy()
            print(key, tag, out[f"{key}_{tag}_text_features"].shape, flush=True)
    for k, v in ZS.items():
        out[f"zs_meta_{k}"] = np.array(v)
    path = os.path.join(HERE, "zsclip.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path) // 1024, "KiB", {k: v.shape for k, v in out.items() if v.ndim})


if __name__ == "__main__":
    main()
