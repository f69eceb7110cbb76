"""The Gemma3 sandwich-norm kernels of norm.hip (residual_norm_fwd, residual_norm_bwd / _bdn / _wg, post_norm_bwd,
rmsnorm_bwd_bdn, rmsnorm_bwd_scatter, the row-mapped rmsnorm_fwd) through their unit-test surface, against plain
fp64 torch on the CPU.

The references restate Gemma3RMSNorm, TF/models/gemma3/modeling_gemma3.py:136-150 (fp32 math, rstd = rsqrt(mean(x^2)
+ eps), scale 1 + w, cast to the input dtype), in the sandwich placement of :399-429 (x = x + post_norm(sublayer(
pre_norm(x)))), with the autocast graph's rounding points the kernels' comments state: y = bf16(norm(t)),
dy = bf16(dR), dt = bf16(...), grad = bf16(grad + bf16(sum)).

The library contracts multiply-adds and reduces in a tree order, so the bar is the derived bound of tests/norm_util.py,
not bit equality: an fp32 output within 2^-17 * M of the fp64 value (M: the sum of the magnitudes of its terms), a bf16
output inside [bf16(r - d), bf16(r + d)] -- bit equality wherever the two ends coincide.  Each stage is checked from the
kernel's own previous output (n and rstd_x from the returned xo, dt and the post-norm weight grad from
bf16(dR returned)), so the bound does not compound.  Before the kernel's output is looked at, each test asserts on
the reference alone that the bf16 interval is a single value on >= 99 % of the elements of y and n and >= 97 % of
dt, so that the bar is bit equality almost everywhere.  Inputs stay in the regime that holds in: t ~ 2 N(0,1)
rounded to bf16, w ~ 0.3 N(0,1), a residual stream with a non-zero mean, dR, dn ~ 0.01 N(0,1); no near-zero rows.

Kernel -> test: residual_norm_fwd_kernel: test_residual_norm_fwd(_without_next_norm); residual_norm_bwd_kernel:
test_residual_norm_bwd_f32_dn; residual_norm_bwd_bdn_kernel: _bf16_dn and _separate_weight_grads (with
rms_wgrad_partial_kernel<f32, bf16> and <bf16, f32>); residual_norm_bwd_wg_kernel + wgrad_finish16_kernel (+
colsum16_kernel at 1029 rows): _fused_weight_grads; post_norm_bwd_kernel: test_post_norm_bwd; rmsnorm_bwd_bdn_kernel:
test_rmsnorm_bwd_bdn; rmsnorm_fwd_kernel with a row map and rmsnorm_bwd_scatter_kernel:
test_rmsnorm_mapped_and_scatter.

Every test also pins: input rows past `rows` (and columns past cols where ld > cols) hold NaN; outputs are
pre-filled with NaN where they must be written and with canaries past `rows`, which must come back unchanged (with
w_next = NULL all of n and rstd_x); a second call on the same inputs gives bit-identical outputs."""
import pytest
import torch

from tests import norm_util as U

pytestmark = pytest.mark.gpu
EPS = 1e-6
PAD = 3           # rows behind `rows` in every buffer
F32, BF16, WG_FUSED, WG_SPLIT = range(4)      # include/ptk.h PTK_RESNORM_BWD_*


def L():
    from projectiontrainer_amd import _lib
    return _lib


def require_single_valued(kind, lo, hi):
    """The condition on the reference alone: the bf16 interval is one value on >= 99 % of the elements of y and n,
    >= 97 % of dt, so the bar is bit equality almost everywhere."""
    f = U.single_valued(lo, hi)
    assert f >= (0.97 if kind == "dt" else 0.99), f"{kind}: the interval is one value on only {f:.4f} of the elements"


def randn(gen, *shape):
    return torch.randn(*shape, generator=gen, dtype=torch.float64)


def out_f32(rows, cols, gpu):
    """NaN where the kernel must write, the canary behind."""
    o = torch.full((rows + PAD, cols), float("nan"))
    o[rows:] = U.CANARY_F32
    return o.to(gpu)


def out_bf16(rows, cols, gpu, written=True):
    o = torch.full((rows + PAD, cols), float("nan"), dtype=torch.bfloat16)
    U.bits(o)[rows if written else 0:] = U.CANARY_BITS
    return o.to(gpu)


def canary_rows_intact(o, rows):
    o = o.cpu()
    if o.dtype == torch.bfloat16:
        return bool((U.bits(o)[rows:] == U.CANARY_BITS).all())
    return bool((o[rows:] == U.CANARY_F32).all())


def same_bits(a, b):
    return torch.equal(a.cpu().view(torch.uint8), b.cpu().view(torch.uint8))


def assert_close_f32(got, r, M, what):
    got = got.double()
    bad = ~((got - r).abs() <= U.REL * M)
    worst = float(torch.nan_to_num((got - r).abs() / M, nan=0.0, posinf=0.0).max())
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} outside 2^-17 M (worst finite |err| / M " \
                                f"{worst:.3e}, NaN: {int(torch.isnan(got).sum())})"


def assert_inside(got, lo, hi, what):
    ok = U.inside(got, lo, hi)
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} of {ok.numel()} outside [bf16(r - d), bf16(r + d)], first at " \
                           f"{(~ok).nonzero()[:4].tolist()} (NaN: {int(torch.isnan(got.double()).sum())})"


# ---------------------------------------------------------------- residual_norm_fwd
# one wave per row, 4 rows per block, NV = ceil(cols / 256) float4 per lane: every NV at its full width and with the
# last column group one lane short, at 5 rows (a ragged second block); the models' widths and the one-lane group
# (4, 260) at 1 / 4 / 37 rows
EVERY_NV = [(5, 256 * nv - d) for nv in range(1, 13) for d in (0, 4)]
FWD_CASES = EVERY_NV + [(1, 1152), (4, 2560), (37, 260), (37, 4), (37, 1152)]


def fwd_inputs(rows, cols):
    gen = torch.Generator().manual_seed(rows * 7919 + cols)
    t = U.bfr(2.0 * randn(gen, rows, cols))
    xi = (0.3 + 2.0 * randn(gen, rows, cols)).float().double()
    w_post, w_next = (0.3 * randn(gen, cols)).float().double(), (0.3 * randn(gen, cols)).float().double()
    return t, xi, w_post, w_next


def fwd_reference(t, xi, w_post, w_next):
    """What can be said before the kernel runs: rstd_t, the interval of y, the interval of xo (fp32 adds of xi and
    the ends of y: monotone), and the condition on y and on n (n from the reference's own xo)."""
    rs_t = U.rstd_ref(t, EPS)
    y = t * rs_t.unsqueeze(1) * (1.0 + w_post)
    ylo, yhi = U.bf16_interval(y, U.REL * y.abs())
    require_single_valued("y", ylo, yhi)
    xo_lo, xo_hi = (xi.float() + ylo.float()).double(), (xi.float() + yhi.float()).double()
    xo_ref = (xi.float() + U.bfr(y).float()).double()
    n_ref = xo_ref * U.rstd_ref(xo_ref, EPS).unsqueeze(1) * (1.0 + w_next)
    require_single_valued("n", *U.bf16_interval(n_ref, U.REL * n_ref.abs()))
    return rs_t, xo_lo, xo_hi


def run_fwd(gpu, t, xi, w_post, w_next, rows, cols):
    lib = L().lib()
    td, xid = U.padded(t.bfloat16(), PAD).to(gpu), U.padded(xi.float(), PAD).to(gpu)
    wp = w_post.float().to(gpu)
    wn = None if w_next is None else w_next.float().to(gpu)
    xo, n = out_f32(rows, cols, gpu), out_bf16(rows, cols, gpu, written=w_next is not None)
    rt = out_f32(rows, 1, gpu)
    rx = out_f32(rows, 1, gpu) if w_next is not None else torch.full((rows + PAD, 1), U.CANARY_F32, device=gpu)
    rc = lib.ptk_residual_norm_fwd(td.data_ptr(), xid.data_ptr(), wp.data_ptr(), L().ptr(wn), xo.data_ptr(),
                                   n.data_ptr(), rt.data_ptr(), rx.data_ptr(), rows, cols, EPS, L().stream_ptr(gpu))
    assert rc == 0, lib.ptk_last_error()
    torch.cuda.synchronize()
    return xo.cpu(), n.cpu(), rt.cpu().flatten(), rx.cpu().flatten()


@pytest.mark.parametrize("rows,cols", FWD_CASES)
def test_residual_norm_fwd(gpu, rows, cols):
    t, xi, w_post, w_next = fwd_inputs(rows, cols)
    rs_t, xo_lo, xo_hi = fwd_reference(t, xi, w_post, w_next)
    xo, n, rt, rx = run_fwd(gpu, t, xi, w_post, w_next, rows, cols)
    assert_close_f32(rt[:rows], rs_t, rs_t, "rstd_t")
    ok = U.inside(xo[:rows], xo_lo, xo_hi)
    assert bool(ok.all()), f"xo: {int((~ok).sum())} outside [xi + bf16(y - d), xi + bf16(y + d)]"
    # the second norm from the returned xo
    xg = xo[:rows].double()
    rs_x = U.rstd_ref(xg, EPS)
    assert_close_f32(rx[:rows], rs_x, rs_x, "rstd_x")
    nr = xg * rs_x.unsqueeze(1) * (1.0 + w_next)
    assert_inside(n[:rows], *U.bf16_interval(nr, U.REL * nr.abs()), "n")
    for o in (xo, n, rt.unsqueeze(1), rx.unsqueeze(1)):
        assert canary_rows_intact(o, rows)
    again = run_fwd(gpu, t, xi, w_post, w_next, rows, cols)
    assert all(same_bits(a, b) for a, b in zip((xo, n, rt, rx), again))


@pytest.mark.parametrize("rows,cols", [(5, 1152), (37, 260), (4, 3068)])
def test_residual_norm_fwd_without_next_norm(gpu, rows, cols):
    """w_next = NULL (the last layer): xo and rstd_t as before, n and rstd_x untouched."""
    t, xi, w_post, w_next = fwd_inputs(rows, cols)
    rs_t, xo_lo, xo_hi = fwd_reference(t, xi, w_post, w_next)
    xo, n, rt, rx = run_fwd(gpu, t, xi, w_post, None, rows, cols)
    assert_close_f32(rt[:rows], rs_t, rs_t, "rstd_t")
    assert bool(U.inside(xo[:rows], xo_lo, xo_hi).all())
    assert canary_rows_intact(n, 0) and canary_rows_intact(rx.unsqueeze(1), 0)
    assert canary_rows_intact(xo, rows) and canary_rows_intact(rt.unsqueeze(1), rows)
    xo_full = run_fwd(gpu, t, xi, w_post, w_next, rows, cols)[0]
    assert same_bits(xo, xo_full)


# ---------------------------------------------------------------- the residual-norm backward, four modes
def bwd_inputs(rows, cols, dn_bf16, salt=0):
    gen = torch.Generator().manual_seed(rows * 104729 + cols * 3 + int(dn_bf16) + 1000003 * salt)
    x2 = (0.3 + 2.0 * randn(gen, rows, cols)).float().double()
    t = U.bfr(2.0 * randn(gen, rows, cols))
    w_pre, w_post = (0.3 * randn(gen, cols)).float().double(), (0.3 * randn(gen, cols)).float().double()
    dn = 0.01 * randn(gen, rows, cols)
    dn = U.bfr(dn) if dn_bf16 else dn.float().double()
    dR = (0.01 * randn(gen, rows, cols)).float().double()
    rs_pre, rs_t = U.rstd_ref(x2, EPS).float().double(), U.rstd_ref(t, EPS).float().double()   # inputs: fp32 values
    g0 = [U.nonzero_g0(cols, gen, scale=2.0 ** -6) for _ in range(2)]
    return dict(x2=x2, t=t, w_pre=w_pre, w_post=w_post, dn=dn, dR=dR, rs_pre=rs_pre, rs_t=rs_t, g0_pre=g0[0],
                g0_post=g0[1])


def run_bwd(gpu, mode, I, rows, cols):
    lib = L().lib()
    dev = lambda t, dt: U.padded(t.to(dt), PAD).to(gpu)
    x2, t = dev(I["x2"], torch.float32), dev(I["t"], torch.bfloat16)
    dn = dev(I["dn"], torch.float32 if mode == F32 else torch.bfloat16)
    rp = dev(I["rs_pre"].unsqueeze(1), torch.float32)
    rt = dev(I["rs_t"].unsqueeze(1), torch.float32)
    wpre, wpost = I["w_pre"].float().to(gpu), I["w_post"].float().to(gpu)
    dR = U.padded(I["dR"].float(), PAD, fill=U.CANARY_F32).to(gpu)
    dt = out_bf16(rows, cols, gpu)
    wg = mode in (WG_FUSED, WG_SPLIT)
    need = lib.ptk_residual_norm_bwd_partial_floats(rows, cols, mode)
    assert (need > 0) == wg
    gp = gq = part = None
    if wg:
        gp, gq = (torch.cat([g, torch.zeros(8, dtype=torch.bfloat16)]) for g in (I["g0_pre"], I["g0_post"]))
        U.bits(gp)[cols:] = U.CANARY_BITS
        U.bits(gq)[cols:] = U.CANARY_BITS
        gp, gq = gp.to(gpu), gq.to(gpu)
        part = torch.full((need + 64,), U.CANARY_F32, device=gpu)
    rc = lib.ptk_residual_norm_bwd(mode, x2.data_ptr(), wpre.data_ptr(), rp.data_ptr(), dn.data_ptr(), dR.data_ptr(),
                                   t.data_ptr(), wpost.data_ptr(), rt.data_ptr(), dt.data_ptr(), rows, cols, L().ptr(gp),
                                   L().ptr(gq), L().ptr(part), need, L().stream_ptr(gpu))
    assert rc == 0, lib.ptk_last_error()
    torch.cuda.synchronize()
    if wg:
        assert bool((part[need:] == U.CANARY_F32).all()), "wrote past the stated partial size"
    return dR.cpu(), dt.cpu(), None if gp is None else gp.cpu(), None if gq is None else gq.cpu()


def check_bwd(gpu, mode, rows, cols):
    I = bwd_inputs(rows, cols, mode != F32)
    # stage A on the inputs; the condition on dt from the reference's own dR
    dx, M = U.rms_bwd_ref(I["x2"], I["w_pre"], I["rs_pre"], I["dn"])
    r, M = I["dR"] + dx, M + I["dR"].abs()
    dt_ref, Mt_ref = U.rms_bwd_ref(I["t"], I["w_post"], I["rs_t"], U.bfr(r))
    require_single_valued("dt", *U.bf16_interval(dt_ref, U.REL * Mt_ref))
    dR, dt, gp, gq = run_bwd(gpu, mode, I, rows, cols)
    assert_close_f32(dR[:rows], r, M, "dR")
    # stage B from bf16(dR returned)
    dy = U.bfr(dR[:rows].double())
    dtr, Mt = U.rms_bwd_ref(I["t"], I["w_post"], I["rs_t"], dy)
    assert_inside(dt[:rows], *U.bf16_interval(dtr, U.REL * Mt), "dt")
    assert canary_rows_intact(dR, rows) and canary_rows_intact(dt, rows)
    if mode in (WG_FUSED, WG_SPLIT):
        for name, g, g0, terms in (("pre", gp, I["g0_pre"], I["dn"] * I["x2"] * I["rs_pre"].unsqueeze(1)),
                                   ("post", gq, I["g0_post"], dy * I["t"] * I["rs_t"].unsqueeze(1))):
            lo, hi = U.acc_interval(g0, terms.sum(dim=0), U.REL * terms.abs().sum(dim=0))
            assert_inside(g[:cols], lo, hi, f"{name}-norm weight grad")
            assert bool((U.bits(g)[cols:] == U.CANARY_BITS).all())
    again = run_bwd(gpu, mode, I, rows, cols)
    assert all(a is None and b is None or same_bits(a, b) for a, b in zip((dR, dt, gp, gq), again))


# the fused mode: every NV at full width and one lane short (5 rows: one full block and a ragged one whose idle
# waves must add zeros), the other row counts, and 1029 rows x 128 columns: 258 partial rows reach colsum16_kernel
@pytest.mark.parametrize("rows,cols", EVERY_NV + [(1, 1152), (4, 260), (37, 2560), (37, 4), (1029, 128)])
def test_residual_norm_bwd_fused_weight_grads(gpu, rows, cols):
    check_bwd(gpu, WG_FUSED, rows, cols)


OTHER = [(1, 4), (4, 260), (5, 1152), (37, 2560), (37, 4), (5, 260), (1, 2560), (4, 1152)]


@pytest.mark.parametrize("rows,cols", OTHER)
def test_residual_norm_bwd_f32_dn(gpu, rows, cols):
    check_bwd(gpu, F32, rows, cols)


@pytest.mark.parametrize("rows,cols", OTHER)
def test_residual_norm_bwd_bf16_dn(gpu, rows, cols):
    check_bwd(gpu, BF16, rows, cols)


# the two separate rms_wgrad passes: also 33 rows (a second 32-row block of one row) and 130
@pytest.mark.parametrize("rows,cols", OTHER + [(33, 1152), (130, 260), (130, 2560), (33, 4)])
def test_residual_norm_bwd_separate_weight_grads(gpu, rows, cols):
    check_bwd(gpu, WG_SPLIT, rows, cols)


# ---------------------------------------------------------------- post_norm_bwd, rmsnorm_bwd_bdn
@pytest.mark.parametrize("rows,cols", OTHER)
def test_post_norm_bwd(gpu, rows, cols):
    lib = L().lib()
    # its own draw (dR here is the grad the last layer's norm receives).  At 37 x 4 the single-valued share of dt
    # is a matter of 3 to 6 of 148 elements; this draw has 3 (the condition is on the reference alone)
    I = bwd_inputs(rows, cols, True, salt=3)
    dy = U.bfr(I["dR"])
    dtr, Mt = U.rms_bwd_ref(I["t"], I["w_post"], I["rs_t"], dy)
    lo, hi = U.bf16_interval(dtr, U.REL * Mt)
    require_single_valued("dt", lo, hi)
    dR, t = U.padded(I["dR"].float(), PAD).to(gpu), U.padded(I["t"].bfloat16(), PAD).to(gpu)
    rt, w = U.padded(I["rs_t"].float().unsqueeze(1), PAD).to(gpu), I["w_post"].float().to(gpu)
    outs = []
    for _ in range(2):
        dt = out_bf16(rows, cols, gpu)
        rc = lib.ptk_post_norm_bwd(dR.data_ptr(), t.data_ptr(), w.data_ptr(), rt.data_ptr(), dt.data_ptr(), rows, cols,
                                   L().stream_ptr(gpu))
        assert rc == 0, lib.ptk_last_error()
        torch.cuda.synchronize()
        outs.append(dt.cpu())
    assert_inside(outs[0][:rows], lo, hi, "dt")
    assert canary_rows_intact(outs[0], rows) and same_bits(*outs)


@pytest.mark.parametrize("dacc", ["none", "separate", "alias"])
@pytest.mark.parametrize("rows,cols", OTHER)
def test_rmsnorm_bwd_bdn(gpu, rows, cols, dacc):
    """dx = dacc + rms_bwd(x, w, rstd, dn bf16); dacc NULL, its own buffer, or dx itself (the first layer's
    input-norm backward accumulates into dR in place)."""
    lib = L().lib()
    I = bwd_inputs(rows, cols, True)
    dx, M = U.rms_bwd_ref(I["x2"], I["w_pre"], I["rs_pre"], I["dn"])
    if dacc != "none":
        dx, M = dx + I["dR"], M + I["dR"].abs()
    x, dn = U.padded(I["x2"].float(), PAD).to(gpu), U.padded(I["dn"].bfloat16(), PAD).to(gpu)
    rs, w = U.padded(I["rs_pre"].float().unsqueeze(1), PAD).to(gpu), I["w_pre"].float().to(gpu)
    outs = []
    for _ in range(2):
        acc = U.padded(I["dR"].float(), PAD, fill=U.CANARY_F32).to(gpu) if dacc != "none" else None
        out = acc if dacc == "alias" else out_f32(rows, cols, gpu)
        rc = lib.ptk_rmsnorm_bwd_bdn(x.data_ptr(), w.data_ptr(), rs.data_ptr(), dn.data_ptr(), L().ptr(acc),
                                     out.data_ptr(), rows, cols, L().stream_ptr(gpu))
        assert rc == 0, lib.ptk_last_error()
        torch.cuda.synchronize()
        outs.append(out.cpu())
        if dacc == "separate":
            assert same_bits(acc, U.padded(I["dR"].float(), PAD, fill=U.CANARY_F32))     # read only
    assert_close_f32(outs[0][:rows], dx, M, "dx")
    assert canary_rows_intact(outs[0], rows) and same_bits(*outs)


# ---------------------------------------------------------------- the row-mapped rmsnorm_fwd and rmsnorm_bwd_scatter
# the loss-row map of the training pass (g = T, gs = Spad, off = Nv - 1: the T rows of each sample that predict a text
# token) and the decode's last-prompt-row map {1, 0, Pp, P - 1}, at tiny sizes
MAPS = {"loss_rows": ((5, 0, 16, 3 - 1), 2 * 5, 2 * 16), "decode": ((1, 0, 12, 7 - 1), 3, 3 * 12)}


@pytest.mark.parametrize("mapname", list(MAPS))
@pytest.mark.parametrize("cols", [4, 260, 1152, 2560])
def test_rmsnorm_mapped_and_scatter(gpu, mapname, cols):
    lib = L().lib()
    m, rows, total = MAPS[mapname]
    src = U.map_rows(m, rows)
    assert int(src.max()) < total and len(set(src.tolist())) == rows
    gen = torch.Generator().manual_seed(cols * 17 + rows)
    ldx = cols + 8
    xs = (0.3 + 2.0 * randn(gen, rows, cols)).float().double()
    w = (0.3 * randn(gen, cols)).float().double()
    rs = U.rstd_ref(xs, EPS)
    y = xs * rs.unsqueeze(1) * (1.0 + w)
    ylo, yhi = U.bf16_interval(y, U.REL * y.abs())
    require_single_valued("n", ylo, yhi)
    x = torch.full((total, ldx), float("nan"))
    x[src, :cols] = xs.float()
    xd, wd = x.to(gpu), w.float().to(gpu)
    outs = []
    for _ in range(2):
        yo, ro = out_bf16(rows, cols, gpu), out_f32(rows, 1, gpu)
        rc = lib.ptk_rmsnorm_mapped(xd.data_ptr(), ldx, L().RowMap(*m), wd.data_ptr(), yo.data_ptr(), ro.data_ptr(),
                                    rows, cols, EPS, L().stream_ptr(gpu))
        assert rc == 0, lib.ptk_last_error()
        torch.cuda.synchronize()
        outs.append((yo.cpu(), ro.cpu()))
    yo, ro = outs[0]
    assert_close_f32(ro[:rows, 0], rs, rs, "rstd")
    assert_inside(yo[:rows], ylo, yhi, "y")
    assert canary_rows_intact(yo, rows) and canary_rows_intact(ro, rows)
    assert same_bits(outs[0][0], outs[1][0]) and same_bits(outs[0][1], outs[1][1])

    # the backward: dR[map(r)] += rms_bwd(x[map(r)], w, rstd[r], dn[r]); every other row of dR bit-unchanged
    dn = (0.01 * randn(gen, rows, cols)).float().double()
    dR0 = (0.01 * randn(gen, total, cols)).float()
    rs_in = rs.float().double()
    dx, M = U.rms_bwd_ref(xs, w, rs_in, dn)
    want, M = dR0[src].double() + dx, M + dR0[src].double().abs()
    xp = torch.full((total, cols), float("nan"))
    xp[src] = xs.float()
    xp, dnd = xp.to(gpu), U.padded(dn.float(), PAD).to(gpu)
    rsd = U.padded(rs_in.float().unsqueeze(1), PAD).to(gpu)
    outs = []
    for _ in range(2):
        dR = dR0.clone().to(gpu)
        rc = lib.ptk_rmsnorm_bwd_scatter(xp.data_ptr(), L().RowMap(*m), wd.data_ptr(), rsd.data_ptr(), dnd.data_ptr(),
                                         dR.data_ptr(), rows, cols, L().stream_ptr(gpu))
        assert rc == 0, lib.ptk_last_error()
        torch.cuda.synchronize()
        outs.append(dR.cpu())
    assert_close_f32(outs[0][src], want, M, "dR rows of the map")
    rest = torch.ones(total, dtype=torch.bool)
    rest[src] = False
    assert same_bits(outs[0][rest], dR0[rest]) and same_bits(*outs)
