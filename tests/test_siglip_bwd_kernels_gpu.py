"""The SigLIP backward's side kernels (csrc/siglip_bwd.hip, the bias grads' column sum of misc.hip) against fp32
torch formulas over the same bf16 inputs, through their stand-alone ABI entries.

Bars (all from the number formats, none from the kernels' own output):
  dx of the LayerNorm backward, dpre of the GELU backward: the kernel computes in fp32 and rounds once, so it may
  differ from bf16(fp32 torch result) only where the two fp32 evaluation orders straddle a bf16 rounding boundary:
  within 1 bf16 ulp on >= 99 % of the elements, within 2 ulp on all.  test_layernorm_bwd_fp32_orders_cpu checks on
  the CPU that a second fp32 evaluation order of the same formula (torch's own layer_norm autograd) stays within
  that bar of the first on these inputs, so the bar is one fp32 reordering can meet.
  dw, db, column sums, position grads: exactly bf16(grad0 + bf16(G)) for some G within rel 1e-5 of the fp64 sum
  (fp32 sums of <= 192 bf16 products in any order stay within ~n 2^-24 of it): the stored value must equal
  bf16(grad0 + bf16(G')) for G' at the lower or the upper end of that interval or in between.
  Every kernel: a repeated call from the same state is bit-identical.
"""
import pytest
import torch
import torch.nn.functional as F

EPS = 1e-6
LN_SHAPES = [(64, 128), (130, 1024), (7, 1152)]


def bf(t):
    return t.to(torch.bfloat16)


def ordered(t):
    """bf16 bit patterns as integers ordered like the values (ulp distances are differences of these)."""
    i = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def ulp_diff(a, b):
    return (ordered(a) - ordered(b)).abs()


def assert_ulp_bar(got, ref_f32, what):
    d = ulp_diff(got.cpu(), bf(ref_f32))
    share = float((d <= 1).float().mean())
    print(f"{what}: within 1 ulp {share:.5f}, max {int(d.max())} ulp")
    assert share >= 0.99 and int(d.max()) <= 2, (what, share, int(d.max()))


def ln_inputs(rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    x = bf(torch.randn(rows, cols, generator=g) * 0.7 + 0.1)
    dy = bf(torch.randn(rows, cols, generator=g) * 0.05)
    w = 1.0 + 0.1 * torch.randn(cols, generator=g)
    dacc = bf(torch.randn(rows, cols, generator=g) * 0.05)
    gw0 = bf(torch.randn(cols, generator=g) * 0.02)
    gb0 = bf(torch.randn(cols, generator=g) * 0.02)
    return x, dy, w, dacc, gw0, gb0


def ln_bwd_formula(x, dy, w, dtype=torch.float32):
    """dx, xhat of the standard LayerNorm backward, every step in `dtype`."""
    x, dy, w = x.to(dtype), dy.to(dtype), w.to(dtype)
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    rstd = torch.rsqrt((xc * xc).mean(-1, keepdim=True) + EPS)
    xh = xc * rstd
    g = dy * w
    dx = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    return dx, xh


def ln_bwd_autograd(x, dy, w):
    xf = x.float().requires_grad_(True)
    F.layer_norm(xf, (x.shape[1],), w.float(), torch.zeros_like(w), EPS).backward(dy.float())
    return xf.grad


@pytest.mark.parametrize("rows,cols", LN_SHAPES)
def test_layernorm_bwd_fp32_orders_cpu(rows, cols):
    """Two fp32 evaluation orders of the LN input gradient (the closed formula and torch's autograd kernel),
    with and without the residual grad added, agree within the bar the GPU kernel is held to."""
    x, dy, w, dacc, _, _ = ln_inputs(rows, cols, 11)
    a, _ = ln_bwd_formula(x, dy, w)
    b = ln_bwd_autograd(x, dy, w)
    assert_ulp_bar(bf(a), b, f"ln_bwd orders {rows}x{cols}")
    assert_ulp_bar(bf(a + dacc.float()), b + dacc.float(), f"ln_bwd orders + dacc {rows}x{cols}")


def assert_accumulated(got, g0, G64, what, rel=1e-5):
    """got == bf16(g0 + bf16(G)) for some G within rel of the fp64 sum G64 (round-to-nearest is monotonic, so
    the result for any such G lies between the results for the interval's two ends)."""
    tol = G64.abs() * rel + 1e-30
    lo = bf(g0.float() + bf((G64 - tol).float()).float())
    hi = bf(g0.float() + bf((G64 + tol).float()).float())
    lo, hi = torch.minimum(ordered(lo), ordered(hi)), torch.maximum(ordered(lo), ordered(hi))
    o = ordered(got.cpu())
    bad = int(((o < lo) | (o > hi)).sum())
    exact = bf(g0.float() + bf(G64.float()).float())
    print(f"{what}: {int((ordered(exact) != o).sum())} of {o.numel()} differ from the fp64 sum's rounding, {bad} outside")
    assert bad == 0, (what, bad)


def _lib():
    from projectiontrainer_amd import _lib as L
    return L, L.lib()


def run_ln_bwd(gpu, x, w, dy, dacc, alias, gw0, gb0):
    L, lib = _lib()
    rows, cols = x.shape
    xd, wd, dyd = x.to(gpu), w.to(gpu), dy.to(gpu)
    gw, gb = gw0.to(gpu).clone(), gb0.to(gpu).clone()
    n = lib.ptk_layernorm_bwd_partial_floats(rows, cols)
    part = torch.empty(n, dtype=torch.float32, device=gpu)
    if alias:
        dx = dacc.to(gpu).clone()
        da = dx
    else:
        dx = torch.full((rows, cols), float("nan"), dtype=torch.bfloat16, device=gpu)
        da = dacc.to(gpu) if dacc is not None else None
    L.check(lib.ptk_layernorm_bwd_bf16(xd.data_ptr(), wd.data_ptr(), dyd.data_ptr(), L.ptr(da), dx.data_ptr(), rows,
                                       cols, EPS, gw.data_ptr(), gb.data_ptr(), part.data_ptr(), n,
                                       L.stream_ptr(gpu)), "ptk_layernorm_bwd_bf16")
    torch.cuda.synchronize()
    return dx, gw, gb


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["plain", "dacc", "alias"])
@pytest.mark.parametrize("rows,cols", LN_SHAPES)
def test_layernorm_bwd(gpu, rows, cols, mode):
    x, dy, w, dacc, gw0, gb0 = ln_inputs(rows, cols, 11)
    use = None if mode == "plain" else dacc
    dx, gw, gb = run_ln_bwd(gpu, x, w, dy, use, mode == "alias", gw0, gb0)
    ref, _ = ln_bwd_formula(x, dy, w)
    if use is not None:
        ref = ref + dacc.float()
    assert_ulp_bar(dx, ref, f"ln_bwd dx {rows}x{cols} {mode}")
    _, xh = ln_bwd_formula(x, dy, w, torch.float64)
    assert_accumulated(gw, gw0, (dy.double() * xh).sum(0), f"ln_bwd dw {rows}x{cols}")
    assert_accumulated(gb, gb0, dy.double().sum(0), f"ln_bwd db {rows}x{cols}")
    dx2, gw2, gb2 = run_ln_bwd(gpu, x, w, dy, use, mode == "alias", gw0, gb0)
    assert torch.equal(dx.view(torch.int16), dx2.view(torch.int16)) and torch.equal(gw, gw2) and torch.equal(gb, gb2)


@pytest.mark.gpu
def test_layernorm_bwd_without_param_grads(gpu):
    """dw = db = NULL: dx alone, no partial scratch needed; one of the two alone is refused before any launch."""
    L, lib = _lib()
    x, dy, w, _, gw0, _ = ln_inputs(64, 128, 11)
    xd, wd, dyd = x.to(gpu), w.to(gpu), dy.to(gpu)
    dx = torch.empty_like(xd)
    L.check(lib.ptk_layernorm_bwd_bf16(xd.data_ptr(), wd.data_ptr(), dyd.data_ptr(), None, dx.data_ptr(), 64, 128, EPS,
                                       None, None, None, 0, L.stream_ptr(gpu)), "ptk_layernorm_bwd_bf16")
    torch.cuda.synchronize()
    assert_ulp_bar(dx, ln_bwd_formula(x, dy, w)[0], "ln_bwd dx only")
    gw = gw0.to(gpu)
    assert lib.ptk_layernorm_bwd_bf16(xd.data_ptr(), wd.data_ptr(), dyd.data_ptr(), None, dx.data_ptr(), 64, 128, EPS,
                                      gw.data_ptr(), None, None, 0, L.stream_ptr(gpu)) == -1


def gelu_tanh_grad_ref(x):
    """d/dx of 0.5 x (1 + tanh(u)), u = k0 (x + k1 x^3) (gelu_pytorch_tanh), in x's dtype, written without the
    cancellation of 1 + tanh(u) and 1 - tanh(u)^2: with s = 0.5 (1 + tanh u) = sigmoid(2 u),
        gelu'(x) = s + x s (1 - s) 2 k0 (1 + 3 k1 x^2).
    (The literal form loses all its digits where tanh(u) -> -1: in fp32 it was more than 1 bf16 ulp from the fp64
    value on 1.1 % of these inputs, x < -4.5, and even the fp64 literal form is 4 % off at x = -6.9.  This form
    agrees with its own fp64 evaluation within 1 ulp on every input here: test_gelu_tanh_grad_reference_cpu.)"""
    k0, k1 = 0.7978845608028654, 0.044715
    s = torch.sigmoid(2 * k0 * (x + k1 * x ** 3))
    return s + x * s * (1 - s) * (2 * k0 * (1 + 3 * k1 * x * x))


GELU_SHAPES = [(64, 256), (3, 4096)]


def gelu_inputs(rows, cols):
    g = torch.Generator().manual_seed(5)
    return bf(torch.randn(rows, cols, generator=g) * 2.0), bf(torch.randn(rows, cols, generator=g) * 0.1)


@pytest.mark.parametrize("rows,cols", GELU_SHAPES)
def test_gelu_tanh_grad_reference_cpu(rows, cols):
    """The fp32 reference formula against its fp64 evaluation and against torch's own fp64 autograd of
    gelu(approximate="tanh") (away from the tail, where that loses its digits too): the reference's own error
    stays inside the bar the kernel is held to."""
    pre, dg = gelu_inputs(rows, cols)
    r32, r64 = dg.float() * gelu_tanh_grad_ref(pre.float()), dg.double() * gelu_tanh_grad_ref(pre.double())
    assert_ulp_bar(bf(r32), r64.float(), f"gelu ref fp32 vs fp64 {rows}x{cols}")
    x = pre.double().requires_grad_(True)
    F.gelu(x, approximate="tanh").backward(dg.double())
    near = pre.float() > -3.0
    assert int(ulp_diff(bf(r64.float()), bf(x.grad.float()))[near].max()) <= 1


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", GELU_SHAPES)
def test_gelu_tanh_bwd(gpu, rows, cols):
    L, lib = _lib()
    pre, dg = gelu_inputs(rows, cols)
    ref = dg.float() * gelu_tanh_grad_ref(pre.float())
    dgd, pred = dg.to(gpu), pre.to(gpu)
    outs = []
    for _ in range(2):
        out = torch.full((rows, cols), float("nan"), dtype=torch.bfloat16, device=gpu)
        L.check(lib.ptk_gelu_tanh_bwd_bf16(dgd.data_ptr(), pred.data_ptr(), out.data_ptr(), rows, cols,
                                           L.stream_ptr(gpu)), "ptk_gelu_tanh_bwd_bf16")
        torch.cuda.synchronize()
        outs.append(out)
    assert_ulp_bar(outs[0], ref, f"gelu_tanh_bwd {rows}x{cols}")
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    # in place (dpre == dg), as ptk_siglip_bwd runs it
    d = dgd.clone()
    L.check(lib.ptk_gelu_tanh_bwd_bf16(d.data_ptr(), pred.data_ptr(), d.data_ptr(), rows, cols,
                                       L.stream_ptr(gpu)), "ptk_gelu_tanh_bwd_bf16")
    torch.cuda.synchronize()
    assert torch.equal(d.view(torch.int16), outs[0].view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", [(128, 384), (192, 1152)])
def test_colsum_acc(gpu, rows, cols):
    L, lib = _lib()
    g = torch.Generator().manual_seed(6)
    x = bf(torch.randn(rows, cols, generator=g) * 0.1)
    g0 = bf(torch.randn(cols, generator=g) * 0.05)
    xd = x.to(gpu)
    outs = []
    for _ in range(2):
        grad = g0.to(gpu).clone()
        part = torch.empty(64 * cols, dtype=torch.float32, device=gpu)
        L.check(lib.ptk_colsum_bf16_acc(xd.data_ptr(), rows, cols, grad.data_ptr(), part.data_ptr(),
                                        part.numel(), L.stream_ptr(gpu)), "ptk_colsum_bf16_acc")
        torch.cuda.synchronize()
        outs.append(grad)
    assert_accumulated(outs[0], g0, x.double().sum(0), f"colsum {rows}x{cols}")
    assert torch.equal(outs[0], outs[1])


@pytest.mark.gpu
def test_pos_grad(gpu):
    L, lib = _lib()
    B, N, D = 3, 64, 128
    g = torch.Generator().manual_seed(7)
    dh0 = bf(torch.randn(B * N, D, generator=g) * 0.1)
    p0 = bf(torch.randn(N, D, generator=g) * 0.05)
    dhd = dh0.to(gpu)
    outs = []
    for _ in range(2):
        dpos = p0.to(gpu).clone()
        L.check(lib.ptk_pos_grad_bf16(dhd.data_ptr(), B, N, D, dpos.data_ptr(), L.stream_ptr(gpu)),
                "ptk_pos_grad_bf16")
        torch.cuda.synchronize()
        outs.append(dpos)
    # three bf16 values summed in index order in fp32
    s = dh0.float().view(B, N, D)
    G = (s[0] + s[1]) + s[2]
    assert torch.equal(outs[0].cpu(), bf(p0.float() + bf(G).float()))
    assert torch.equal(outs[0], outs[1])
