"""Stage 2 with a trainable projector on the HIP path vs the reference: mode B (LLM and projector trained) and
mode C (LLM frozen, projector trained).

`tests/golden/s2p*_tiny{,_bf16}.npz` come from the reference's own VQATrainerStage2.train() with
`freeze_projection_layer=False` (tests/golden/make_golden_stage2_proj.py).  The engine replays the same collated
batches; every bar follows tests/test_stage2_gpu.py's rule (the fixtures are fp32 / bf16 twins):
  micro-batch loss |d| <= 2e-2;  accumulated grads rel-L2 <= max(2e-2, 2 x twin distance), cos >= min(0.999,
  1 - 4 (1 - twin cos));  both pre-clip norms within the same relative bar;  LR equal to 1e-12;
  params after each AdamW step: max |d| <= 2.5 * sum(lr) + 1 bf16 ulp, median |d| <= 0.05 * lr + half an ulp
-- on the projector's four tensors and, in mode B, on every LLM tensor.
"""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import golden_util as G
from tests.test_stage2_gpu import cosine, load, record, rel_l2, stored

pytestmark = pytest.mark.gpu

SETS = ["s2p_tiny", "s2pf_tiny", "s2pf2_tiny"]


def build(meta, gpu, **kw):
    from projectiontrainer_amd import weights as W
    from projectiontrainer_amd.config import PRESETS
    from projectiontrainer_amd.gemma3 import Gemma3CausalLM
    from projectiontrainer_amd.projectors import MLPProjector
    from projectiontrainer_amd.siglip import SiglipVisionTower
    from projectiontrainer_amd.stage2 import Stage2Engine
    cfg = PRESETS["tiny"]
    vp, lp = W.siglip_vision_params(cfg.vision), W.gemma3_params(cfg.text)
    pp = W.projector_params(cfg.vision.hidden_size, cfg.text.hidden_size, cfg.expansion_factor)
    if meta["precision"] == "bf16":     # the reference casts the towers and the projector to bf16
        vp = {k: G.bf16_round(v) for k, v in vp.items()}
        lp = {k: G.bf16_round(v) for k, v in lp.items()}
        pp = {k: G.bf16_round(v) for k, v in pp.items()}
    proj = MLPProjector(cfg.vision.hidden_size, cfg.text.hidden_size)
    proj.load_state_dict({k: torch.from_numpy(v) for k, v in pp.items()})   # (a trained one: the engine rounds it)
    proj.to(gpu)
    total = meta["max_train_steps"]
    train_llm = meta.get("mode", "A") != "C"
    kw.setdefault("train_llm", train_llm)
    kw.setdefault("train_projector", meta.get("mode", "A") != "A")
    llm = Gemma3CausalLM(cfg.text, lp, gpu, max_pos=256, frozen=not kw["train_llm"])
    eng = Stage2Engine(SiglipVisionTower(cfg.vision, vp, gpu), llm, proj, learning_rate=meta["lr"],
                       weight_decay=meta["weight_decay"], gradient_accumulation_steps=meta["gas"],
                       max_grad_norm=meta["max_grad_norm"], warmup_steps=math.ceil(meta["warmup_ratio"] * total),
                       total_steps=total, **kw)
    return cfg, eng


def batches(d, meta, gpu):
    """(pixels, question ids, answer ids, sync) per recorded micro-batch."""
    from projectiontrainer_amd import weights as W
    from projectiontrainer_amd.config import PRESETS
    items = W.synthetic_vqa_items(PRESETS["tiny"], meta["n_items"], meta["seed"])
    px = torch.stack([it["pixel_values"] for it in items])
    per_epoch = math.ceil(meta["n_items"] / meta["batch_size"])
    for m in range(meta["micro_batches"]):
        i = m % per_epoch
        yield (px[d[f"m{m}_order"]].to(gpu), torch.from_numpy(d[f"m{m}_question_input_ids"]).to(gpu),
               torch.from_numpy(d[f"m{m}_answer_input_ids"]).to(gpu),
               (i + 1) % meta["gas"] == 0 or i + 1 == per_epoch)


def check_grads(t, d, base, twin, prefix, names, grads):
    for n in names:
        key = f"{prefix}.{n}"
        ref, sr, sc = stored(d, key)
        got = grads[n] if key in d.files else G.sub_sample(grads[n], sr, sc)
        nb, _, _ = stored(base, key)
        nt, _, _ = stored(twin, key)
        tol_r = max(2e-2, 2.0 * rel_l2(nt, nb))
        tol_c = min(0.999, 1.0 - 4.0 * (1.0 - cosine(nt, nb)))
        r, c = rel_l2(got, ref), cosine(got, ref)
        record(t, key, rel_l2=r, cos=c, tol_rel_l2=tol_r, tol_cos=tol_c)
        print(f"{t} {key}: rel-L2 {r:.3e} (<= {tol_r:.3e}) cos {c:.6f} (>= {tol_c:.6f})")
        assert r <= tol_r and c >= tol_c, (key, r, tol_r, c, tol_c)


def check_norm(t, d, base, twin, key, got):
    ref = float(d[key])
    tol = max(2e-2, 2.0 * abs(float(twin[key]) - float(base[key])) / float(base[key]))
    r = abs(got - ref) / ref
    record(t, key, rel=r, tol=tol)
    print(f"{t} {key}: {got:.6f} vs {ref:.6f} rel {r:.3e} (<= {tol:.3e})")
    assert r <= tol, (key, got, ref, tol)


def check_params(t, d, prefix, names, params, lr_sum, lr):
    for n in names:
        key = f"{prefix}.{n}"
        ref, sr, sc = stored(d, key)
        got = G.sub_sample(params[n], sr, sc) if key not in d.files else params[n]
        ulp = 2.0 ** (np.floor(np.log2(max(np.abs(ref).max(), 1e-30))) - 7)
        mx, md = np.abs(got - ref).max(), np.median(np.abs(got - ref))
        record(t, key, max_abs=mx, median_abs=md, atol=2.5 * lr_sum + ulp)
        assert mx <= 2.5 * lr_sum + ulp, (key, mx, 2.5 * lr_sum + ulp)
        assert md <= 0.05 * lr + ulp / 2, (key, md)


def host(sd):
    return {k: v.float().cpu().numpy() for k, v in sd.items()}


@pytest.mark.parametrize("name", [s + p for s in SETS for p in ("_bf16", "")])
def test_stage2_proj_vs_reference_golden(gpu, name):
    d, meta = load(name)
    base, _ = load(name.replace("_bf16", ""))
    twin, _ = load(name.replace("_bf16", "") + "_bf16")
    cfg, eng = build(meta, gpu)
    mode_b = meta["mode"] == "B"
    assert (eng.state is not None) == mode_b and eng.pstate is not None
    pn, ln = meta["proj_param_names"], meta["param_names"]
    t = f"stage2_proj[{name}]"
    o, lr_sum = 0, 0.0
    for m, (px, q, a, sync) in enumerate(batches(d, meta, gpu)):
        loss = float(eng.forward_backward(px, q, a))
        dl = abs(loss - float(d[f"m{m}_loss"]))
        record(t, f"m{m}_loss", abs=dl)
        print(f"{t} m{m}_loss: {loss:.6f} vs {float(d[f'm{m}_loss']):.6f}")
        assert dl <= 2e-2, (m, loss, float(d[f"m{m}_loss"]))
        if not sync:
            continue
        torch.cuda.synchronize()
        check_grads(t, d, base, twin, f"o{o}_proj_grad", pn, host(eng.projector_state_dict(grads=True)))
        if mode_b:
            check_grads(t, d, base, twin, f"o{o}_grad", ln, host(eng.state.state_dict_hf(grads=True)))
        eng.optimizer_step()
        torch.cuda.synchronize()
        assert abs(eng.last_lr - float(d[f"o{o}_lr"])) <= 1e-12, (o, eng.last_lr, float(d[f"o{o}_lr"]))
        lr_sum += eng.last_lr
        check_norm(t, d, base, twin, f"o{o}_proj_grad_norm", float(eng.proj_grad_norm))
        check_params(t, d, f"o{o}_proj_param", pn, host(eng.projector_state_dict()), lr_sum, meta["lr"])
        assert not eng.pstate.grad.any()          # zeroed for the next accumulation
        if mode_b:
            check_norm(t, d, base, twin, f"o{o}_grad_norm", float(eng.grad_norm))
            check_params(t, d, f"o{o}_param", ln, host(eng.state.state_dict_hf()), lr_sum, meta["lr"])
        o += 1
    assert o == meta["opt_steps"]


def test_mode_c_builds_no_llm_state_and_leaves_the_llm_alone(gpu):
    """A frozen LLM gets no Gemma3TrainState (no grad buffer, no moments), keeps the k-step-tiled weights it was
    built with, and every one of its tensors is bit-identical after training steps; validation sees the updated
    projector."""
    d, meta = load("s2pf_tiny_bf16")
    cfg, eng = build(meta, gpu)
    assert eng.state is None and eng.exp_avg.numel() == 0 and eng.llm.frozen
    for lay in eng.llm.layers:     # (a shape without a tiled copy has none in a frozen model either)
        assert (lay["wqkv_kt"] is None) == bool(lay["wqkv"].shape[0] % 16 or lay["wqkv"].shape[1] % 32)
    keys = [k for k, v in eng.llm.layers[0].items() if torch.is_tensor(v)]
    snap = lambda: [eng.llm.embed.clone(), eng.llm.final_norm.clone()] + [lay[k].clone() for lay in eng.llm.layers
                                                                         for k in keys]
    before = snap()
    bl = list(batches(d, meta, gpu))
    v0 = float(eng.forward_loss(*bl[0][:3]))
    for px, q, a, _ in bl[:3]:
        eng.forward_backward(px, q, a)
        eng.optimizer_step()
    torch.cuda.synchronize()
    for x, y in zip(before, snap()):
        assert torch.equal(x, y)
    assert float(eng.grad_norm) == 0.0 and float(eng.proj_grad_norm) > 0.0
    assert float(eng.forward_loss(*bl[0][:3])) != v0


def test_default_mode_is_untouched(gpu):
    """An engine built with the defaults and one with train_llm=True, train_projector=False passed explicitly:
    bit-identical loss, LLM grads and LLM parameters over the s2_tiny_bf16 batches, and no projector state."""
    d, meta = load("s2_tiny_bf16")
    runs = []
    for explicit in (False, True):
        cfg, eng = build(dict(meta, mode="A"), gpu) if explicit else _build_default(meta, gpu)
        assert eng.pstate is None
        out = []
        for px, q, a, sync in batches(d, meta, gpu):
            out.append(eng.forward_backward(px, q, a).clone())
            if sync:
                out.append(eng.state.grad.clone())
                eng.optimizer_step()
                out.append(eng.state.flat.clone())
        torch.cuda.synchronize()
        runs.append(out)
    assert len(runs[0]) == len(runs[1])
    for x, y in zip(*runs):
        assert torch.equal(x, y)


def _build_default(meta, gpu):
    """tests/test_stage2_gpu.py's build: no mode argument at all."""
    from tests.test_stage2_gpu import build as build_a
    return build_a(meta["name"], gpu, meta)


@pytest.mark.parametrize("name", ["s2p_tiny_bf16", "s2pf2_tiny_bf16"])
def test_optimizer_state_roundtrip_with_projector(gpu, name):
    """optimizer_state() carries the projector's moments; a fresh engine that loads it continues bit-identically;
    a state of another layout is refused."""
    d, meta = load(name)
    bl = list(batches(d, meta, gpu))
    _, eng = build(meta, gpu)
    for px, q, a, sync in bl[:2]:
        eng.forward_backward(px, q, a)
    eng.optimizer_step()
    sd = eng.optimizer_state()
    assert sd["proj_numel"] == eng.pstate.numel and sd["proj_exp_avg"].any() and sd["proj_exp_avg_sq"].any()
    _, eng2 = build(meta, gpu)
    eng2.load_optimizer_state(sd)
    assert torch.equal(eng2.pstate.exp_avg, eng.pstate.exp_avg) and torch.equal(eng2.exp_avg, eng.exp_avg)
    assert (eng2.opt_step, eng2.sched_step) == (1, 1)
    eng2.pstate.flat.copy_(eng.pstate.flat)
    eng2.pstate.refresh()
    if eng.state is not None:
        eng2.state.flat.copy_(eng.state.flat)
        eng2.state.refresh()
    for e in (eng, eng2):
        e.forward_backward(*bl[2][:3])
        e.optimizer_step()
    torch.cuda.synchronize()
    assert torch.equal(eng2.pstate.flat, eng.pstate.flat) and torch.equal(eng2.pstate.exp_avg_sq, eng.pstate.exp_avg_sq)
    # another layout: a mode-A engine's state has no projector moments; and the other way round
    a_meta = dict(meta, mode="A")
    _, eng_a = build(a_meta, gpu)
    with pytest.raises(ValueError):
        eng.load_optimizer_state(eng_a.optimizer_state())
    with pytest.raises(ValueError):
        eng_a.load_optimizer_state(sd)


@pytest.mark.parametrize("freeze_llm", [False, True], ids=["mode_B", "mode_C"])
def test_save_model_writes_the_reference_layout(gpu, tmp_path, freeze_llm):
    """VQATrainerStage2 driven with the reference's flags (--unfreeze_projection_layer, the LLM trained or frozen):
    one epoch, then the checkpoint of Stage2/trainer.py:721-769 -- language_model/ only when the LLM was trained,
    projection_layer/model.safetensors + projector_config.json when the projector was; the projector directory
    reloads through the reference's recipe (config JSON, then the first .safetensors file of the directory) to the
    engine's parameters bit for bit."""
    import types
    from safetensors.torch import load_file
    from transformers import Gemma3ForCausalLM, Gemma3TextConfig, SiglipConfig, SiglipModel
    from projectiontrainer_amd import weights as W
    from projectiontrainer_amd import dist as D
    from projectiontrainer_amd.config import PRESETS, to_hf_dicts
    from projectiontrainer_amd.projectors import MLPProjector
    from projectiontrainer_amd.vqa_trainer import VQATrainerStage2
    cfg = PRESETS["tiny"]
    vis_kw, txt_kw = to_hf_dicts(cfg)
    sig = SiglipModel(SiglipConfig(text_config=dict(vocab_size=64, hidden_size=64, intermediate_size=128,
                                                    num_hidden_layers=1, num_attention_heads=1,
                                                    max_position_embeddings=16, bos_token_id=None, eos_token_id=None,
                                                    pad_token_id=None), vision_config=vis_kw))
    sig.load_state_dict({k: torch.from_numpy(v) for k, v in W.siglip_vision_params(cfg.vision).items()}, strict=False)
    llm = Gemma3ForCausalLM(Gemma3TextConfig(**txt_kw))
    llm.load_state_dict({k: torch.from_numpy(v) for k, v in W.gemma3_params(cfg.text).items()}, strict=False)
    proj = MLPProjector(cfg.vision.hidden_size, cfg.text.hidden_size)
    pp = W.projector_params(cfg.vision.hidden_size, cfg.text.hidden_size)
    proj.load_state_dict({k: torch.from_numpy(v) for k, v in pp.items()})
    data = W.synthetic_vqa_items(cfg, 6, seed=21)
    tok = types.SimpleNamespace(pad_token_id=0, eos_token_id=1, padding_side="left")
    logs = []
    tr = VQATrainerStage2(D.DistState(2), sig.to(torch.bfloat16), llm.to(torch.bfloat16), proj, tok, data, data[:2],
                          str(tmp_path), 2, 1e-3, 0.01, 1, 2, 0.05, freeze_vision_encoder=True,
                          freeze_projection_layer=False, freeze_llm=freeze_llm, enable_qlora=False,
                          train_ve_first_epoch=False, wandb_project="x", log_fn=lambda d, s: logs.append(d))
    assert (tr.engine.state is None) == freeze_llm and tr.language_model.frozen == freeze_llm
    tr.train()
    torch.cuda.synchronize()
    assert tr.global_step == 2
    assert len([x for x in logs if "train/batch_loss" in x]) == 3 and len([x for x in logs if "val/loss" in x]) == 1
    ck = tmp_path / "checkpoint-epoch_1"
    assert (ck / "language_model" / "model.safetensors").exists() == (not freeze_llm)
    pdir = ck / "projection_layer"
    assert sorted(os.listdir(pdir)) == ["model.safetensors", "projector_config.json"]
    # the reference's load_pretrained_projector recipe (Stage2/train_vqa_stage2.py:25-80)
    text = (pdir / "projector_config.json").read_text()
    conf = json.loads(text)
    assert conf == {"vision_dim": cfg.vision.hidden_size, "llm_dim": cfg.text.hidden_size}
    assert text == json.dumps(conf, indent=4)
    files = [f for f in os.listdir(pdir) if f.endswith((".bin", ".safetensors")) and "optimizer" not in f
             and "scheduler" not in f]
    sd = load_file(str(pdir / next(f for f in files if f.endswith(".safetensors"))), device="cpu")
    fresh = MLPProjector(conf["vision_dim"], conf["llm_dim"])
    res = fresh.load_state_dict(sd)
    assert not res.missing_keys and not res.unexpected_keys
    eng_sd = tr.engine.projector_state_dict()
    moved = False
    for k, v in eng_sd.items():
        assert sd[k].dtype == torch.bfloat16 and torch.equal(sd[k], v.cpu()), k
        assert torch.equal(fresh.state_dict()[k], v.float().cpu()), k
        assert torch.equal(tr.projection_layer.state_dict()[k].cpu(), v.float().cpu()), k
        moved |= not torch.equal(v.float().cpu(), G_bf16(pp[k]))
    assert moved                                                   # the projector was trained
    st = torch.load(str(ck / "optimizer_rank0.pt"), weights_only=True)
    assert torch.equal(st["proj_exp_avg"], tr.engine.pstate.exp_avg.cpu()) and st["proj_exp_avg"].any()
    assert (st["step"], st["sched_step"]) == (2, 2)


def G_bf16(a):
    return torch.from_numpy(G.bf16_round(a))


@pytest.mark.parametrize("train_llm", [True, False], ids=["mode_B", "mode_C"])
def test_world2_projector_replicas_match_single_process(gpu, train_llm):
    """World 2 over gloo on one device: the projector's grads are all-reduced whole and each rank takes the same
    AdamW step, so both replicas are bit-identical; and they equal one process that accumulates both halves of
    the batch and scales the grad by 1/2 (at W = 2 the two bf16 grad sums round identically; the bars are
    test_stage2_zero1_ranks_match_single_process's for W = 2, the tied embedding within 2 lr)."""
    import tempfile
    import torch.multiprocessing as mp
    from tests import stage2_proj_worker
    from tests.test_dist import _port
    from projectiontrainer_amd import weights as W
    from projectiontrainer_amd.config import PRESETS
    from projectiontrainer_amd.stage2 import synthetic_engine
    world = 2
    with tempfile.TemporaryDirectory() as td:
        mp.spawn(stage2_proj_worker.stage2_proj, args=(world, _port(), td, train_llm), nprocs=world, join=True)
        pj = [np.load(f"{td}/proj{r}.npy") for r in range(world)]
        pn = [np.load(f"{td}/projnorm{r}.npy") for r in range(world)]
        if train_llm:
            ll = [np.load(f"{td}/llm{r}.npy") for r in range(world)]
            ln = np.load(f"{td}/llmnorm0.npy")
    np.testing.assert_array_equal(pj[0], pj[1])
    np.testing.assert_array_equal(pn[0], pn[1])
    cfg = PRESETS["tiny"].replace(batch_size=2 * world, text_len=8 + 12, question_len=8)
    torch.manual_seed(0)
    eng = synthetic_engine(cfg, gpu, seed=3, learning_rate=1e-3, total_steps=10, train_llm=train_llm,
                           train_projector=True)
    start = eng.pstate.flat.float().cpu().numpy()
    px, q, a = (torch.from_numpy(t).to(gpu) for t in W.synthetic_vqa_batch(cfg, seed=9))
    for r in range(world):
        sl = slice(2 * r, 2 * r + 2)
        eng.forward_backward(px[sl], q[sl], a[sl])
    eng.pstate.grad.mul_(1.0 / world)
    if train_llm:
        eng.state.grad.mul_(1.0 / world)
    eng.optimizer_step()
    torch.cuda.synchronize()
    assert eng.sched_step == 1
    one = eng.pstate.flat.float().cpu().numpy()
    assert (one != start).any()
    np.testing.assert_array_equal(one, pj[0])
    np.testing.assert_allclose(float(eng.proj_grad_norm), float(pn[0][0]), rtol=1e-6)
    if train_llm:
        np.testing.assert_array_equal(ll[0], ll[1])
        flat = eng.state.flat.float().cpu().numpy()
        n = min(flat.size, ll[0].size)
        e0 = eng.state.offsets["embed"][0]
        e1 = e0 + cfg.text.vocab_size * cfg.text.hidden_size
        mask = np.ones(n, dtype=bool)
        mask[e0:e1] = False
        assert np.abs(flat[e0:e1] - ll[0][e0:e1]).max() <= 2 * 1e-3 + 1e-3
        np.testing.assert_array_equal(flat[:n][mask], ll[0][:n][mask])
        np.testing.assert_allclose(float(eng.grad_norm), float(ln[0]), rtol=1e-6)
