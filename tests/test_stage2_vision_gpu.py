"""Stage2Engine(train_vision=True): the SigLIP tower trained through the engine, with the LLM and the projector
trained or frozen.  Synthetic tiny towers (stage2.synthetic_engine); the vision side has 64 patches (image 128,
patch 16, head_dim 64), which the tower's backward needs and config.py's tiny preset does not have."""
import pytest
import torch

from tests.test_optim_gpu import bf16_ulp, bits

pytestmark = pytest.mark.gpu

HP = dict(learning_rate=1e-3, weight_decay=0.01, max_grad_norm=1.0, total_steps=10)
# (train_llm, train_projector); (False, False) is the tower alone
MODES = {"llm": (True, False), "llm_proj": (True, True), "proj": (False, True), "vision_only": (False, False)}


def config(batch=2):
    from projectiontrainer_amd.config import GEMMA3_TINY, SiglipVisionConfig, Stage1Config
    vis = SiglipVisionConfig(image_size=128, patch_size=16, hidden_size=128, num_attention_heads=2,
                             intermediate_size=256, num_hidden_layers=2)
    return Stage1Config(vision=vis, text=GEMMA3_TINY, batch_size=batch, text_len=8 + 12, question_len=8)


def engine(gpu, mode, train_vision, **kw):
    from projectiontrainer_amd.stage2 import synthetic_engine
    train_llm, train_projector = MODES[mode]
    torch.manual_seed(0)
    return synthetic_engine(config(), gpu, seed=3, train_llm=train_llm, train_projector=train_projector,
                            train_vision=train_vision, **dict(HP, **kw))


def batch(gpu, seed=9):
    from projectiontrainer_amd import weights as W
    return tuple(torch.from_numpy(t).to(gpu) for t in W.synthetic_vqa_batch(config(), seed=seed))


@pytest.mark.parametrize("mode", list(MODES))
def test_train_vision_changes_nothing_else_and_equals_the_tower_backward(gpu, mode):
    """The loss and the LLM and projector grads are bit-identical to the same engine with the tower frozen; the
    tower's grads are SiglipVisionTower.backward of the engine's own d(last_hidden_state), whose patch-0 rows are
    zero.  The tower alone has no frozen-tower engine to compare with (nothing would be trainable, and an engine
    that trains the LLM or the projector holds that module's parameters rounded to bf16): its loss is compared
    with its own validation loss, which takes the frozen forward."""
    b = batch(gpu)
    ev = engine(gpu, mode, True)
    assert ev.vstate is not None and ev.vision_trainable
    if mode == "vision_only":
        e0 = engine(gpu, "proj", False)
        l0 = ev.forward_loss(*b).clone()
    else:
        e0 = engine(gpu, mode, False)
        l0 = e0.forward_backward(*b).clone()
    assert e0.vstate is None
    lv = ev.forward_backward(*b).clone()
    torch.cuda.synchronize()
    assert torch.equal(l0.view(torch.int32), lv.view(torch.int32)) and float(lv) > 0
    if MODES[mode][0]:
        assert e0.state.grad.any() and torch.equal(bits(e0.state.grad), bits(ev.state.grad))
    else:
        assert ev.state is None
    if MODES[mode][1]:
        assert e0.pstate.grad.any() and torch.equal(bits(e0.pstate.grad), bits(ev.pstate.grad))
    else:
        assert ev.pstate is None
    cfg = config()
    N, D = cfg.vision.num_patches, cfg.vision.hidden_size
    d_out = ev.dvis.view(cfg.batch_size, N, D)
    assert not d_out[:, 0].any() and d_out[:, 1:].any()
    got = ev.vstate.grad.clone()
    assert got.any()
    ev.vstate.zero_grad()
    ev.vision.backward(ev.dvis, ev.vstate)
    torch.cuda.synchronize()
    assert torch.equal(bits(got), bits(ev.vstate.grad))
    sd = ev.vision_state_dict(grads=True)
    assert sd["vision_model.embeddings.patch_embedding.weight"].shape == (D, 3, 16, 16)
    assert all(v.any() for k, v in sd.items() if "k_proj.bias" not in k), [k for k, v in sd.items() if not v.any()]
    with pytest.raises(ValueError):
        e0.vision_state_dict()


def torch_adamw_step(p0, g, lr, max_norm):
    """torch's clip_grad_norm_ + single-tensor AdamW on CPU bf16 tensors (tests/test_optim_gpu.py's reference)."""
    p = torch.nn.Parameter(p0.cpu().clone())
    p.grad = g.cpu().clone()
    norm = torch.nn.utils.clip_grad_norm_([p], max_norm, foreach=False)
    opt = torch.optim.AdamW([p], lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=HP["weight_decay"], foreach=False)
    opt.step()
    return p.data, float(norm)


@pytest.mark.parametrize("mode", ["llm_proj", "vision_only"])
def test_optimizer_step_is_torch_adamw_with_the_towers_own_clip(gpu, mode):
    """After optimizer_step the tower's store is torch's bf16 AdamW step from the engine's grads, clipped on the
    tower's own norm: tests/test_optim_gpu.py's bar (within one bf16 ulp at |p|; step 1 from zero moments is
    bit-identical), the parameters moved, vision_grad_norm is that norm, and the grads are zeroed."""
    ev = engine(gpu, mode, True)
    ev.forward_backward(*batch(gpu))
    p0, g = ev.vstate.flat.clone(), ev.vstate.grad.clone()
    small0 = ev.vision.pos.clone()
    ev.optimizer_step()
    torch.cuda.synchronize()
    want, norm = torch_adamw_step(p0, g, ev.last_lr, HP["max_grad_norm"])
    got = ev.vstate.flat.cpu()
    d = (got.double() - want.double()).abs()
    over = int((d > bf16_ulp(p0.cpu())).sum())
    print(f"tower AdamW [{mode}]: {int((d > 0).sum())} of {got.numel()} differ, {over} by more than one ulp; "
          f"norm {float(ev.vision_grad_norm)!r} vs {norm!r}")
    assert over == 0
    assert torch.equal(bits(got), bits(want))
    assert not torch.equal(bits(got), bits(p0))
    torch.testing.assert_close(float(ev.vision_grad_norm), norm, rtol=1e-6, atol=0)
    assert not ev.vstate.grad.any() and ev.opt_step == 1
    # the fp32 copies the forward reads were refreshed from the store
    assert not torch.equal(ev.vision.pos, small0)
    assert torch.equal(ev.vision.pos, ev.vstate.view("pos").float())
    if mode == "llm_proj":   # each module on its own norm
        assert float(ev.grad_norm) > 0 and float(ev.proj_grad_norm) > 0
        assert len({float(ev.grad_norm), float(ev.proj_grad_norm), float(ev.vision_grad_norm)}) == 3


def test_set_vision_trainable_false_freezes_the_tower_and_keeps_its_state(gpu):
    """Frozen again, a step takes the frozen forward (the saved-activation workspace is not touched), leaves the
    tower's store and moments bit-unchanged and still trains the LLM; unfrozen, the tower trains on."""
    ev = engine(gpu, "llm", True)
    b = batch(gpu)
    ev.forward_backward(*b)
    ev.optimizer_step()
    flat, m, v = ev.vstate.flat.clone(), ev.vstate.exp_avg.clone(), ev.vstate.exp_avg_sq.clone()
    assert m.any() and v.any()
    ev.set_vision_trainable(False)
    ws = ev.vstate.workspace(config().batch_size)
    ws.fill_(0x5A)
    llm0 = ev.state.flat.clone()
    ev.forward_backward(*b)
    ev.optimizer_step()
    torch.cuda.synchronize()
    assert bool((ws == 0x5A).all())
    assert torch.equal(bits(ev.vstate.flat), bits(flat)) and torch.equal(bits(ev.vstate.exp_avg), bits(m))
    assert torch.equal(bits(ev.vstate.exp_avg_sq), bits(v)) and not ev.vstate.grad.any()
    assert not torch.equal(bits(ev.state.flat), bits(llm0)) and ev.opt_step == 2
    ev.set_vision_trainable(True)
    ev.forward_backward(*b)
    ev.optimizer_step()
    torch.cuda.synchronize()
    assert not torch.equal(bits(ev.vstate.flat), bits(flat)) and ev.opt_step == 3
    with pytest.raises(ValueError):
        engine(gpu, "llm", False).set_vision_trainable(True)


def test_two_micro_batches_accumulate_before_one_step(gpu):
    """gas = 2: the second micro-batch's grads are added to the first's as autograd adds into a bf16 .grad,
    bf16(g1 + bf16(G2)), with bf16(G2) what the same micro-batch leaves from zeroed grads."""
    b1, b2 = batch(gpu, 9), batch(gpu, 10)
    ea = engine(gpu, "llm", True, gradient_accumulation_steps=2)
    ea.forward_backward(*b1)
    g1 = ea.vstate.grad.clone()
    ea.forward_backward(*b2)
    g12 = ea.vstate.grad.clone()
    eb = engine(gpu, "llm", True, gradient_accumulation_steps=2)
    eb.forward_backward(*b2)
    g2 = eb.vstate.grad.clone()
    torch.cuda.synchronize()
    assert g1.any() and g2.any() and not torch.equal(bits(g1), bits(g2))
    assert torch.equal(bits(g12), bits((g1.float() + g2.float()).to(torch.bfloat16)))
    p0 = ea.vstate.flat.clone()
    ea.optimizer_step()
    torch.cuda.synchronize()
    assert ea.opt_step == 1 and not torch.equal(bits(ea.vstate.flat), bits(p0)) and not ea.vstate.grad.any()


def test_optimizer_state_round_trip_carries_the_towers_moments(gpu):
    b = batch(gpu)
    ev = engine(gpu, "llm_proj", True)
    ev.forward_backward(*b)
    ev.optimizer_step()
    sd = ev.optimizer_state()
    assert sd["vision_numel"] == ev.vstate.numel and sd["vision_exp_avg"].any() and sd["vision_exp_avg_sq"].any()
    e2 = engine(gpu, "llm_proj", True)
    e2.load_optimizer_state(sd)
    for dst, src in ((e2.vstate, ev.vstate), (e2.pstate, ev.pstate), (e2.state, ev.state)):
        dst.flat.copy_(src.flat)
        dst.refresh()
    assert (e2.opt_step, e2.sched_step) == (ev.opt_step, ev.sched_step) == (1, 1)
    for e in (ev, e2):
        e.forward_backward(*batch(gpu, 10))
        e.optimizer_step()
    torch.cuda.synchronize()
    for x, y in ((e2.vstate.flat, ev.vstate.flat), (e2.vstate.exp_avg, ev.vstate.exp_avg),
                 (e2.vstate.exp_avg_sq, ev.vstate.exp_avg_sq), (e2.state.flat, ev.state.flat),
                 (e2.pstate.flat, ev.pstate.flat)):
        assert torch.equal(bits(x), bits(y))
    with pytest.raises(ValueError):      # a state without the tower's moments is another layout
        ev.load_optimizer_state(engine(gpu, "llm_proj", False).optimizer_state())
    with pytest.raises(ValueError):
        engine(gpu, "llm_proj", False).load_optimizer_state(sd)
