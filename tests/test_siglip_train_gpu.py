"""The trained SigLIP tower on the HIP path (ptk_siglip_train_fwd / ptk_siglip_bwd through SiglipVisionTower and
SiglipTrainState) and the projector's input gradient (ptk_projector_input_grad).

Reference: fp32 torch autograd on the CPU through the repository's own restatement of the tower,
oracle.stage1_ref.siglip_vision_forward (parity-pinned to the reference's forward); the twin is the same function
in bf16.  Tolerance, per gradient tensor (tests/test_stage2_proj_gpu.py's rule; both sides of the bar come from
the two references, never from the code under test):
    rel-L2 <= max(2e-2, 2 x twin rel-L2),  cosine >= min(0.999, 1 - 4 (1 - twin cosine)).
"""
import functools

import numpy as np
import pytest
import torch

from tests import golden_util as G
from tests.test_stage2_gpu import cosine, record, rel_l2

pytestmark = pytest.mark.gpu


def vision_cfg(image=128, layers=2):
    from projectiontrainer_amd.config import SiglipVisionConfig
    return SiglipVisionConfig(image_size=image, patch_size=16, hidden_size=128, num_attention_heads=2,
                              intermediate_size=256, num_hidden_layers=layers)


CASES = {"tiny_b2": (128, 2, 2), "tiny_b3": (128, 2, 3), "seq576_b1": (384, 1, 1)}   # image, layers, batch


def params(cfg):
    """bf16-representable HF-named parameters (the reference loads the tower in bf16)."""
    from projectiontrainer_amd import weights as W
    return {k: G.bf16_round(v) for k, v in W.siglip_vision_params(cfg).items()}


def inputs(cfg, B, seed=3):
    g = torch.Generator().manual_seed(seed)
    px = (torch.rand(B, 3, cfg.image_size, cfg.image_size, generator=g) * 2 - 1).to(torch.bfloat16)
    d_out = (torch.randn(B, cfg.num_patches, cfg.hidden_size, generator=g) * 0.05).to(torch.bfloat16)
    d_out[:, 0] = 0          # last_hidden_state[:, 1:] drops patch 0
    return px, d_out


@functools.lru_cache(maxsize=None)
def reference(case):
    """{name: grad} of fp32 autograd and of its bf16 twin, computed once per case and shared."""
    from oracle import stage1_ref as R
    image, layers, B = CASES[case]
    cfg = vision_cfg(image, layers)
    px, d_out = inputs(cfg, B)
    out = []
    for dtype in (torch.float32, torch.bfloat16):
        p = {k: torch.from_numpy(v).clone().requires_grad_(True) for k, v in params(cfg).items()}
        y = R.siglip_vision_forward(p, cfg, px.float(), dtype=dtype)
        y.backward(d_out.to(dtype))
        out.append({k: v.grad.double().numpy() for k, v in p.items()})
    return out


def build(cfg, gpu, train=True):
    from projectiontrainer_amd.siglip import SiglipVisionTower
    from projectiontrainer_amd.stage2 import SiglipTrainState
    tower = SiglipVisionTower(cfg, params(cfg), gpu)
    return tower, (SiglipTrainState(tower) if train else None)


def run(tower, state, px, d_out, gpu):
    out = torch.empty((px.shape[0] * tower.cfg.num_patches, tower.cfg.hidden_size), dtype=torch.bfloat16, device=gpu)
    tower.forward_train_into(px.to(gpu), out, state)
    tower.backward(d_out.to(gpu).view(-1, tower.cfg.hidden_size), state)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_train_forward_is_bit_identical_to_frozen(gpu, case):
    image, layers, B = CASES[case]
    cfg = vision_cfg(image, layers)
    px, _ = inputs(cfg, B)
    frozen, _ = build(cfg, gpu, train=False)
    tower, state = build(cfg, gpu)
    shape = (B * cfg.num_patches, cfg.hidden_size)
    a, b, c = (torch.full(shape, float("nan"), dtype=torch.bfloat16, device=gpu) for _ in range(3))
    frozen.forward_into(px.to(gpu), a)          # k-step-tiled frozen weights, no state
    tower.forward_into(px.to(gpu), b)           # the rebound tower's frozen path (row-major weights)
    tower.forward_train_into(px.to(gpu), c, state)
    torch.cuda.synchronize()
    assert not torch.isnan(a.float()).any()
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert torch.equal(a.view(torch.int16), c.view(torch.int16))


def check_grads(gpu, case, select):
    image, layers, B = CASES[case]
    cfg = vision_cfg(image, layers)
    px, d_out = inputs(cfg, B)
    base, twin = reference(case)
    tower, state = build(cfg, gpu)
    run(tower, state, px, d_out, gpu)
    got = {k: v.float().cpu().double().numpy() for k, v in state.state_dict_hf(grads=True).items()}
    assert set(got) == set(base)
    bad, keys = [], [k for k in sorted(base) if select(k)]
    assert keys
    for k in keys:
        tol_r = max(2e-2, 2.0 * rel_l2(twin[k], base[k]))
        tol_c = min(0.999, 1.0 - 4.0 * (1.0 - cosine(twin[k], base[k])))
        r, c = rel_l2(got[k], base[k]), cosine(got[k], base[k])
        record(f"siglip_train[{case}]", k, rel_l2=r, cos=c, tol_rel_l2=tol_r, tol_cos=tol_c,
               norm=np.linalg.norm(got[k]), ref_norm=np.linalg.norm(base[k]), twin_norm=np.linalg.norm(twin[k]))
        print(f"{case} {k}: rel-L2 {r:.3e} (<= {tol_r:.3e}) cos {c:.6f} (>= {tol_c:.6f}) |got| "
              f"{np.linalg.norm(got[k]):.3e} |ref| {np.linalg.norm(base[k]):.3e} |twin| {np.linalg.norm(twin[k]):.3e}")
        if not (r <= tol_r and c >= tol_c):
            bad.append((k, r, tol_r, c, tol_c))
    assert not bad, bad
    return got


def is_key_bias(k):
    return k.endswith("self_attn.k_proj.bias")


@pytest.mark.parametrize("case", list(CASES))
def test_grads_vs_autograd(gpu, case):
    """Every parameter grad under the twin rule, through state_dict_hf(grads=True) against autograd in HF names.

    The key projections' bias grads are under the same rule, and are also checked to be exactly zero: their exact
    gradient is zero for every input (a key bias adds q . b_k to every score of a query's row, which softmax does
    not see), the fp32 reference and the twin hold only rounding residue there (norms ~1e-8 and ~5e-5, next to
    ~5e-2 for the query bias of the same layer), and ptk_siglip_bwd adds nothing to them.  (Summing dK's columns
    instead left 1.4e-4 at 576 patches -- rel-L2 1.514e4 against the rule's 1.099e4 there -- because the flash
    backward's delta = rowsum(dO . O) comes from the bf16-rounded O, so the rows of d(scores) do not sum to zero.)"""
    got = check_grads(gpu, case, lambda k: True)
    kb = [k for k in got if is_key_bias(k)]
    assert kb and all(not got[k].any() for k in kb)
    assert all(got[k].any() for k in got if not is_key_bias(k))


def test_backward_accumulates_and_repeats(gpu):
    """From zeroed grads one call leaves bf16(0 + bf16(G)) = bf16(G); a second call from the same activations must
    leave bf16(g + bf16(G)) = bf16(g + g), elementwise.  A whole repeated run from zeroed grads is bit-identical."""
    cfg = vision_cfg()
    px, d_out = inputs(cfg, 2)
    tower, state = build(cfg, gpu)
    out1 = run(tower, state, px, d_out, gpu)
    g1 = state.grad.clone()
    assert g1.float().abs().sum() > 0
    tower.backward(d_out.to(gpu).view(-1, cfg.hidden_size), state)
    torch.cuda.synchronize()
    expect = (g1.float() + g1.float()).to(torch.bfloat16)
    assert torch.equal(state.grad.view(torch.int16), expect.view(torch.int16))
    state.zero_grad()
    out2 = run(tower, state, px, d_out, gpu)
    assert torch.equal(out1.view(torch.int16), out2.view(torch.int16))
    assert torch.equal(state.grad.view(torch.int16), g1.view(torch.int16))


def test_kernel_refusals_reach_python(gpu):
    """196 patches (B/16-224's grid) are refused with the limit named, before any launch."""
    from projectiontrainer_amd import _lib as L
    from projectiontrainer_amd.config import SiglipVisionConfig
    cfg = SiglipVisionConfig(image_size=224, patch_size=16, hidden_size=128, num_attention_heads=2,
                             intermediate_size=256, num_hidden_layers=1)
    tower, state = build(cfg, gpu)
    px, _ = inputs(cfg, 1)
    out = torch.empty((196, 128), dtype=torch.bfloat16, device=gpu)
    with pytest.raises(L.PtkError, match="multiple of 64"):
        tower.forward_train_into(px.to(gpu), out, state)


# ------------------------------------------------------------------ projector input gradient
ROWS, DV, DL = 128, 128, 128


def proj_params():
    from projectiontrainer_amd import weights as W
    return {k: G.bf16_round(v) for k, v in W.projector_params(DV, DL).items()}


def proj_inputs():
    g = torch.Generator().manual_seed(9)
    x = (torch.randn(ROWS, DV, generator=g) * 0.5).to(torch.bfloat16)
    dy = (torch.randn(ROWS, DL, generator=g) * 0.05).to(torch.bfloat16)
    return x, dy


@functools.lru_cache(maxsize=None)
def proj_reference():
    from oracle import stage1_ref as R
    x, dy = proj_inputs()
    out = []
    for dtype in (torch.float32, torch.bfloat16):
        pp = {k: torch.from_numpy(v).to(dtype) for k, v in proj_params().items()}
        xx = x.to(dtype).requires_grad_(True)
        R.projector_forward(pp, xx).backward(dy.to(dtype))
        out.append(xx.grad.double().numpy())
    return out


@pytest.mark.parametrize("trained", [False, True])
def test_projector_input_grad(gpu, trained):
    from projectiontrainer_amd import _lib as L
    from projectiontrainer_amd.projectors import MLPProjector
    from projectiontrainer_amd.stage2 import PROJ_KEYS, ProjectorTrainState
    lib = L.lib()
    proj = MLPProjector(DV, DL)
    proj.load_state_dict({k: torch.from_numpy(v) for k, v in proj_params().items()})
    proj.to(gpu)
    x, dy = (t.to(gpu) for t in proj_inputs())
    I = proj.inter_dim
    ps = ProjectorTrainState(proj, gpu) if trained else None
    c = ps.c if trained else proj.desc()
    a, h = (torch.empty((ROWS, I), dtype=torch.bfloat16, device=gpu) for _ in range(2))
    y = torch.empty((ROWS, DL), dtype=torch.float32, device=gpu)
    st = L.stream_ptr(gpu)
    L.check(lib.ptk_projector_fwd(c, ROWS, x.data_ptr(), a.data_ptr(), h.data_ptr(), y.data_ptr(), L.RowMap(0, 0, 0, 0),
                                  DL, 1, st), "ptk_projector_fwd")
    ws = torch.empty(lib.ptk_projector_input_grad_workspace_bytes(c, ROWS), dtype=torch.uint8, device=gpu)
    dvis = torch.full((ROWS, DV), float("nan"), dtype=torch.bfloat16, device=gpu)
    gp = [None] * 4
    if trained:
        # the four grads of a plain ptk_projector_bwd_bf16 call from the same (non-zero) starting grads
        ps.grad.copy_((torch.randn(ps.numel, generator=torch.Generator().manual_seed(4)) * 0.01).to(torch.bfloat16))
        g0 = ps.grad.clone()
        gp = [t.data_ptr() for t in ps.state_dict(grads=True).values()]
        L.check(lib.ptk_projector_bwd_bf16(c, ROWS, x.data_ptr(), a.data_ptr(), h.data_ptr(), dy.data_ptr(), *gp,
                                           ws.data_ptr(), ws.numel(), st), "ptk_projector_bwd_bf16")
        torch.cuda.synchronize()
        plain = ps.grad.clone()
        ps.grad.copy_(g0)
    L.check(lib.ptk_projector_input_grad(c, ROWS, x.data_ptr(), a.data_ptr(), h.data_ptr(), dy.data_ptr(), *gp,
                                         dvis.data_ptr(), ws.data_ptr(), ws.numel(), st), "ptk_projector_input_grad")
    torch.cuda.synchronize()
    if trained:
        assert not torch.equal(plain, g0)
        assert torch.equal(ps.grad.view(torch.int16), plain.view(torch.int16))
        assert list(ps.state_dict(grads=True)) == list(PROJ_KEYS)
    base, twin = proj_reference()
    got = dvis.float().cpu().double().numpy()
    tol_r = max(2e-2, 2.0 * rel_l2(twin, base))
    tol_c = min(0.999, 1.0 - 4.0 * (1.0 - cosine(twin, base)))
    r, cs = rel_l2(got, base), cosine(got, base)
    record(f"projector_input_grad[trained={trained}]", "dx_vis", rel_l2=r, cos=cs, tol_rel_l2=tol_r, tol_cos=tol_c)
    print(f"dx_vis trained={trained}: rel-L2 {r:.3e} (<= {tol_r:.3e}) cos {cs:.6f} (>= {tol_c:.6f})")
    assert r <= tol_r and cs >= tol_c
