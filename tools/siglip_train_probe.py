"""Stage-timer spans of the trained SigLIP tower: siglip.fwd (ptk_siglip_train_fwd) and siglip.bwd
(ptk_siglip_bwd) with their sub-stages, in ms per step, and the training workspace's size.

    python tools/siglip_train_probe.py [--batch 32] [--steps 5] [--warmup 2] [--layers 24] [--out FILE.json]

Random-init SigLIP-L/16-384 (no checkpoints offline); d_out is random with its patch-0 rows zero.  The spans are
device events around the launches (csrc/stages.cpp), nested: siglip.fwd contains siglip.embed / .attn / .flash /
.mlp / .post_norm, siglip.bwd contains siglip.bwd.post_norm / .mlp / .attn (which contains .flash) / .embed.
"""
import argparse
import dataclasses
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from projectiontrainer_amd import _lib as L
    from projectiontrainer_amd.config import SIGLIP_L16_384
    from projectiontrainer_amd.siglip import SiglipVisionTower
    from projectiontrainer_amd.stage2 import SiglipTrainState
    dev = torch.device("cuda:0")
    cfg = dataclasses.replace(SIGLIP_L16_384, num_hidden_layers=a.layers)
    tower = SiglipVisionTower.random_init(cfg, dev, seed=0)
    state = SiglipTrainState(tower)
    B, N, D = a.batch, cfg.num_patches, cfg.hidden_size
    g = torch.Generator(device=dev).manual_seed(1)
    px = (torch.rand((B, 3, cfg.image_size, cfg.image_size), generator=g, device=dev) * 2 - 1).to(torch.bfloat16)
    d_out = (torch.randn((B, N, D), generator=g, device=dev) * 0.01).to(torch.bfloat16)
    d_out[:, 0] = 0
    d_out = d_out.view(B * N, D)
    out = torch.empty((B * N, D), dtype=torch.bfloat16, device=dev)
    ws = state.workspace(B)
    for i in range(a.warmup + a.steps):
        if i == a.warmup:
            torch.cuda.synchronize()
            L.stage_timers_enable(True)
        tower.forward_train_into(px, out, state)
        tower.backward(d_out, state)
    torch.cuda.synchronize()
    t = L.stage_timers_read(reset=True)
    L.stage_timers_enable(False)
    ms = {k: v[0] / a.steps for k, v in t.items()}
    res = {"config": "SigLIP-L/16-384", "layers": a.layers, "batch": B, "rows": B * N, "steps": a.steps,
           "train_workspace_bytes": int(ws.numel()),
           "frozen_workspace_bytes": int(L.lib().ptk_siglip_workspace_bytes(tower.c_cfg, B)),
           "ms_per_step": ms,
           "bwd_over_fwd": ms["siglip.bwd"] / ms["siglip.fwd"] if ms.get("siglip.fwd") else None,
           "grad_finite": bool(torch.isfinite(state.grad.float()).all()), "grad_nonzero": bool(state.grad.any())}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
