"""ptk_projector_bwd_bf16: the Stage-2 projector backward in the reference's bf16 numerics (bf16 parameters, the
four grads accumulated into a bf16 .grad as autograd does, bf16(grad + bf16(G))).

Reference: torch autograd, on the same device, of the same nn.Sequential held in bf16 under
torch.autocast(bfloat16), from zero grads.  Bars: those of test_projector_weight_grads_tn_vs_fp32 (rel-L2 < 1.5e-2,
cosine > 0.9999 per tensor); rounding a result once to bf16 adds about 2^-9 / sqrt(3) ~ 1.1e-3, which fits inside.
Shapes (rows, patches per image N, Dv, I, Dl): under one 64-row K step (the fixtures' 2 x 16 patches); ragged; a
multiple of 64 (the TN path); the widths and row alignment of a real run (B x 576 rows), where the census must show
the TN GEMM.  Rows 0, N, 2N, ... of dy are zero (the dropped patch 0)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(32, 16, 128, 1280, 128), (100, 25, 64, 640, 128), (192, 64, 64, 640, 128),
          (1152, 576, 1024, 10240, 1152)]
KEYS = ("model.0.weight", "model.0.bias", "model.2.weight", "model.2.bias")


class Case:
    """One shape: the bf16 store, the forward's saved activations, dy and a workspace."""

    def __init__(self, gpu, rows, N, Dv, I, Dl):
        from projectiontrainer_amd import _lib as L
        from projectiontrainer_amd.projectors import MLPProjector
        from projectiontrainer_amd.stage2 import ProjectorTrainState
        torch.manual_seed(rows)
        self.L, self.rows = L, rows
        self.ps = ps = ProjectorTrainState(MLPProjector(Dv, Dl, expansion_factor=I // Dv), gpu)
        bf = torch.bfloat16
        self.x = torch.randn(rows, Dv, device=gpu).to(bf)
        self.a = torch.empty(rows, I, dtype=bf, device=gpu)
        self.h = torch.empty(rows, I, dtype=bf, device=gpu)
        out = torch.empty(rows, Dl, dtype=torch.float32, device=gpu)
        L.check(L.lib().ptk_projector_fwd(ps.c, rows, self.x.data_ptr(), self.a.data_ptr(), self.h.data_ptr(),
                                          out.data_ptr(), L.RowMap(0, 0, 0, 0), Dl, 1, L.stream_ptr(gpu)), "fwd")
        dy = torch.randn(rows, Dl, device=gpu) * 0.05
        dy[::N] = 0
        self.dy = dy.to(bf)
        self.ws = torch.empty(L.lib().ptk_projector_bwd_bf16_workspace_bytes(ps.c, rows), dtype=torch.uint8, device=gpu)
        self.gpu = gpu

    def call(self, ws_bytes=None, null=None):
        L, ps = self.L, self.ps
        g = [ps.view(k, ps.grad).data_ptr() for k in KEYS]
        if null is not None:
            g[null] = None
        return L.lib().ptk_projector_bwd_bf16(ps.c, self.rows, self.x.data_ptr(), self.a.data_ptr(), self.h.data_ptr(),
                                              self.dy.data_ptr(), *g, self.ws.data_ptr(),
                                              self.ws.numel() if ws_bytes is None else ws_bytes,
                                              L.stream_ptr(self.gpu))

    def run(self, start=None):
        """The grad store after one call from `start` (None: zeros)."""
        ps = self.ps
        if start is None:
            ps.grad.zero_()
        else:
            ps.grad.copy_(start)
        self.L.check(self.call(), "ptk_projector_bwd_bf16")
        torch.cuda.synchronize()
        return ps.grad.clone()

    def reference(self):
        ps = self.ps
        Dv, I, Dl = ps.dims
        ref = torch.nn.Sequential(torch.nn.Linear(Dv, I), torch.nn.GELU(), torch.nn.Linear(I, Dl)).to(self.gpu)
        ref = ref.to(torch.bfloat16)
        ref.load_state_dict({k[len("model."):]: v for k, v in ps.state_dict().items()})
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = ref(self.x)
        y.backward(self.dy)
        return {"model." + k: p.grad for k, p in ref.named_parameters()}


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "x".join(map(str, s)))
def case(gpu, request):
    c = Case(gpu, *request.param)
    yield c
    del c
    torch.cuda.empty_cache()


def test_grads_vs_torch_bf16_autograd(case):
    L, ps = case.L, case.ps
    L.gemm_path_counts(reset=True)
    case.run()
    paths = {p for p, _ in L.gemm_path_counts(reset=True)}
    if case.rows == 1152:     # a real run's row alignment (B x 576): both weight grads on the TN GEMM, in place
        assert "tn" in paths, paths
    ref = case.reference()
    for k in KEYS:
        g, r = ps.view(k, ps.grad).float(), ref[k].float()
        rel = float((g - r).norm() / r.norm())
        cos = float(F.cosine_similarity(g.flatten(), r.flatten(), dim=0))
        print(f"rows {case.rows} {k}: rel-L2 {rel:.3e} cos {cos:.6f}")
        assert rel < 1.5e-2, (k, rel)
        assert cos > 0.9999, (k, cos)
    # the gaps between the store's segments belong to no tensor and stay zero
    used = torch.zeros(ps.numel, dtype=torch.bool, device=case.gpu)
    for k in KEYS:
        off, shape = ps.offsets[k]
        used[off:off + ps.view(k).numel()] = True
    assert not ps.grad[~used].any()


def test_accumulation_is_exact_and_deterministic(case):
    """grad = bf16(grad + bf16(G)) in all four tensors: from grads preloaded with g0 the call gives exactly
    (g0 + gz) rounded once, gz being the result from zero grads; and a repeated call from the same state gives
    the same bits (no floating-point atomics)."""
    ps = case.ps
    gz = case.run()
    assert torch.equal(gz, case.run())
    torch.manual_seed(7)
    g0 = torch.zeros_like(gz)
    for k in KEYS:     # random grads of each tensor's own scale
        v = ps.view(k, gz)
        ps.view(k, g0).copy_(torch.randn(v.shape, device=case.gpu) * v.float().std())
    got = case.run(g0)
    want = (g0.float() + gz.float()).bfloat16()
    for k in KEYS:
        assert torch.equal(ps.view(k, got), ps.view(k, want)), k
    assert torch.equal(got, case.run(g0))


def test_error_returns_before_any_launch(gpu):
    c = Case(gpu, 100, 25, 64, 640, 128)
    L, ps = c.L, c.ps
    ps.grad.fill_(1.0)
    before = ps.grad.clone()
    L.gemm_path_counts(reset=True)
    assert c.call(ws_bytes=c.ws.numel() - 1) != 0
    assert b"workspace" in L.lib().ptk_last_error()
    for i in range(4):
        assert c.call(null=i) != 0
        assert b"null" in L.lib().ptk_last_error()
    torch.cuda.synchronize()
    assert not L.gemm_path_counts(reset=True)
    assert torch.equal(ps.grad, before)
    # dims that are no multiple of 8 are refused too
    bad = L.ProjectorC.from_buffer_copy(ps.c)
    bad.llm_dim = 124
    assert L.lib().ptk_projector_bwd_bf16(bad, c.rows, c.x.data_ptr(), c.a.data_ptr(), c.h.data_ptr(),
                                          c.dy.data_ptr(), *[ps.view(k, ps.grad).data_ptr() for k in KEYS],
                                          c.ws.data_ptr(), c.ws.numel(), L.stream_ptr(gpu)) != 0
    assert torch.equal(ps.grad, before)
