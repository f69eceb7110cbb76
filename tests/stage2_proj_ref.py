"""fp32 CPU restatement of the reference's Stage-2 step with a TRAINABLE projector (a test helper, not a test).

Composed from the pinned oracle functions only (oracle/stage1_ref.py, oracle/stage2_ref.py):
  mode B  LLM and projector trained    (freeze_llm=False, freeze_projection_layer=False)
  mode C  LLM frozen, projector trained (freeze_llm=True,  freeze_projection_layer=False)
The vision tower runs under no_grad; the projector runs with grad (Stage2/trainer.py:336-337); loss / gas twice
(:422 and Accelerator.backward), grads summed over micro-batches; at a sync each trainable module is clipped on
its own norm to 1.0 (:437-439), then one AdamW step over all of them with the shared LR, and the cosine schedule.
"""
from __future__ import annotations

import math

import torch

from oracle import stage1_ref as R
from oracle import stage2_ref as S


class Module:
    """fp32 parameters of one trainable module + its AdamW moments."""
    def __init__(self, params):
        self.params = {k: torch.as_tensor(v).float().clone().requires_grad_(True) for k, v in params.items()}
        self.exp_avg = {k: torch.zeros_like(v) for k, v in self.params.items()}
        self.exp_avg_sq = {k: torch.zeros_like(v) for k, v in self.params.items()}


def loss_fn(vp, vcfg, llm_params, lcfg, proj_params, pixel_values, q_ids, a_ids, pad_id):
    with torch.no_grad():
        patch = R.siglip_vision_forward(vp, vcfg, pixel_values)[:, 1:, :]
    proj = R.projector_forward(proj_params, patch.float())
    E = llm_params["model.embed_tokens.weight"]
    x, mask, labels = S.stage2_inputs(proj, E, q_ids, a_ids, pad_id, math.sqrt(lcfg.hidden_size))
    hidden = R.gemma3_forward(llm_params, lcfg, x, mask)
    return R.causal_lm_loss(hidden, E, labels)


def train(vp, vcfg, lp, lcfg, pp, batches, *, train_llm, gas, lr0, warmup, total, pad_id, weight_decay=0.01,
          max_norm=1.0):
    """Replays collated micro-batches (a list per epoch).  Returns the per-micro-batch losses and the per-step
    records {lr, grad_norm (LLM, mode B), proj_grad_norm, grads, params, proj_grads, proj_params}."""
    llm = Module(lp) if train_llm else None
    llm_params = llm.params if train_llm else {k: torch.as_tensor(v).float() for k, v in lp.items()}
    proj = Module(pp)
    step = sched = 0
    losses, steps = [], []
    for epoch_batches in batches:
        for i, b in enumerate(epoch_batches):
            loss = loss_fn(vp, vcfg, llm_params, lcfg, proj.params, b["pixel_values"], b["question_input_ids"],
                           b["answer_input_ids"], pad_id)
            ((loss / gas) / gas).backward()
            losses.append(float(loss.detach()))
            if not ((i + 1) % gas == 0 or i + 1 == len(epoch_batches)):
                continue
            lr = lr0 * R.cosine_lambda(sched, warmup, total)
            rec = {"lr": lr}
            for mod, tag in ((llm, ""), (proj, "proj_")):
                if mod is None:
                    continue
                grads = {k: p.grad.detach().clone() for k, p in mod.params.items()}
                rec[tag + "grads"] = {k: g.clone() for k, g in grads.items()}
                rec[tag + "grad_norm"] = float(R.clip_grad_norm_(list(grads.values()), max_norm))
                ts = R.TrainState({k: p.detach() for k, p in mod.params.items()}, mod.exp_avg, mod.exp_avg_sq, step)
                with torch.no_grad():
                    R.adamw_step(ts, grads, lr, weight_decay=weight_decay)
                for p in mod.params.values():
                    p.grad = None
                rec[tag + "params"] = {k: p.detach().clone() for k, p in mod.params.items()}
            step += 1
            sched += 1
            steps.append(rec)
    return losses, steps
