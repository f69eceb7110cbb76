"""Pin the fp32 restatement of Stage 2 with a trainable projector (tests/stage2_proj_ref.py) to the reference's
own VQA trainer.

`tests/golden/s2p*_tiny.npz` come from Stage2/trainer.py:VQATrainerStage2.train() on CPU with
`freeze_projection_layer=False` (tests/golden/make_golden_stage2_proj.py): s2p (mode B: LLM and projector trained,
gas 2), s2pf (mode C: LLM frozen, gas 1, 6 steps), s2pf2 (mode C, gas 2).  The bars are tests/test_stage2_oracle.py's:
losses rtol 1e-4; LR rtol 1e-12; both grad norms rtol 1e-4; accumulated grads rtol 1e-3 with an absolute floor of
2e-4 x the tensor's rms; params after AdamW within 0.05 lr."""
import math

import numpy as np
import pytest
import torch

from oracle import stage2_ref as S
from projectiontrainer_amd import weights as W
from projectiontrainer_amd.config import PRESETS
from tests import golden_util as G
from tests import stage2_proj_ref as P
from tests.test_stage2_oracle import fixture_batches, load, rms

FP32 = ["s2p_tiny", "s2pf_tiny", "s2pf2_tiny"]
ALL = FP32 + [n + "_bf16" for n in FP32]


@pytest.mark.parametrize("name", ALL)
def test_stage2_proj_fixture_contract(name):
    """Weights regenerate bit-identically; each recorded batch is vqa_collate_fn of the samples in the recorded
    order; the meta names the mode and gas the file name stands for."""
    d, meta = load(name)
    cfg = PRESETS["tiny"]
    vp, lp = W.siglip_vision_params(cfg.vision), W.gemma3_params(cfg.text)
    pp = W.projector_params(cfg.vision.hidden_size, cfg.text.hidden_size, cfg.expansion_factor)
    np.testing.assert_array_equal(G.fingerprint(vp, lp, pp), d["weight_fingerprint"])
    items = W.synthetic_vqa_items(cfg, meta["n_items"], meta["seed"])
    for m in range(meta["micro_batches"]):
        b = S.collate([items[i] for i in d[f"m{m}_order"]], cfg.text.pad_token_id, meta["padding_side"])
        np.testing.assert_array_equal(b["question_input_ids"].numpy(), d[f"m{m}_question_input_ids"])
        np.testing.assert_array_equal(b["answer_input_ids"].numpy(), d[f"m{m}_answer_input_ids"])
    base = name.replace("_bf16", "")
    want = {"s2p_tiny": ("B", 2, 4), "s2pf_tiny": ("C", 1, 6), "s2pf2_tiny": ("C", 2, 4)}[base]
    assert (meta["mode"], meta["gas"], meta["opt_steps"]) == want
    assert meta["precision"] == ("bf16" if name.endswith("_bf16") else "no")
    assert bool(meta["param_names"]) == (meta["mode"] == "B")      # LLM tensors in mode B only
    for k in ("torch", "transformers", "accelerate"):
        assert meta[k]


@pytest.mark.parametrize("name", ["s2pf_tiny", "s2pf_tiny_bf16"])
def test_projector_clip_engaged_and_idle(name):
    """The gas-1 frozen-LLM fixtures exercise both branches of the projector's clip: its recorded pre-clip norm
    lies above max_grad_norm at some steps and below it at others."""
    d, meta = load(name)
    norms = [float(d[f"o{o}_proj_grad_norm"]) for o in range(meta["opt_steps"])]
    assert max(norms) > meta["max_grad_norm"] and min(norms) < meta["max_grad_norm"], norms


@pytest.mark.parametrize("name", FP32)
def test_stage2_proj_restatement_matches_reference(name):
    torch.set_num_threads(8)
    d, meta = load(name)
    cfg = PRESETS["tiny"]
    vp, lp = W.siglip_vision_params(cfg.vision), W.gemma3_params(cfg.text)
    pp = {k: torch.from_numpy(v) for k, v in W.projector_params(cfg.vision.hidden_size, cfg.text.hidden_size).items()}
    total = meta["max_train_steps"]
    warmup = math.ceil(meta["warmup_ratio"] * total)
    losses, steps = P.train({k: torch.from_numpy(v) for k, v in vp.items()}, cfg.vision, lp, cfg.text, pp,
                            fixture_batches(d, meta), train_llm=meta["mode"] == "B", gas=meta["gas"],
                            lr0=meta["lr"], warmup=warmup, total=total, pad_id=cfg.text.pad_token_id)
    assert len(losses) == meta["micro_batches"] and len(steps) == meta["opt_steps"]
    for m, l in enumerate(losses):
        np.testing.assert_allclose(l, float(d[f"m{m}_loss"]), rtol=1e-4)
    for o, rec in enumerate(steps):
        np.testing.assert_allclose(rec["lr"], float(d[f"o{o}_lr"]), rtol=1e-12)
        np.testing.assert_allclose(rec["proj_grad_norm"], float(d[f"o{o}_proj_grad_norm"]), rtol=1e-4)
        for n in meta["proj_param_names"]:
            g = rec["proj_grads"][n]
            G.check_tensor(d, f"o{o}_proj_grad.{n}", g, 1e-3, max(1e-8, 2e-4 * rms(g)))
            G.check_tensor(d, f"o{o}_proj_param.{n}", rec["proj_params"][n], 1e-5, 0.05 * meta["lr"])
        if meta["mode"] == "B":
            np.testing.assert_allclose(rec["grad_norm"], float(d[f"o{o}_grad_norm"]), rtol=1e-4)
            for n in meta["param_names"]:
                g = rec["grads"][n]
                G.check_tensor(d, f"o{o}_grad.{n}", g, 1e-3, max(1e-8, 2e-4 * rms(g)))
                G.check_tensor(d, f"o{o}_param.{n}", rec["params"][n], 1e-5, 0.05 * meta["lr"])
        else:
            assert f"o{o}_grad_norm" not in d.files
