"""The RMSNorm and q/k-norm weight-grad block of train.hip (rms_wgrad_partial_kernel in its three type pairs,
colsum16_kernel, wgrad_finish16_kernel, both qknorm_wgrad_partial kernels) through its unit-test surface, bit-exact.

The operation (TF/models/gemma3/modeling_gemma3.py:136-150: y = x * rstd * (1 + w), so dw[c] = sum_r dy[r, c] *
x[r, c] * rstd[r]; q_norm / k_norm sit under the rotate-half RoPE, :356-360 and :208-258) with the autocast graph's
rounding points the kernels' comments state: dy = bf16(dR) where dy_round is set, grad = bf16(grad + bf16(sum)).

rstd and the cos / sin tables are inputs here, so the data are chosen exactly representable: x, qkv, dQ, dK and the
partials small integers, dy integer multiples of 2^-8, rstd in {1, 1/2, 1/4, 1/8} varying by row, cos / sin in
{-1, 0, 1/2, 1}.  Every product and every partial sum is then an integer multiple of a power of two (the "unit")
below 2^24 units -- each test asserts that on the reference, for the sum of the terms' magnitudes -- so neither the
tree order of the kernels' sums nor FMA contraction can change an fp32 result, and bf16(g0 + bf16(S)) must be
bit-equal to the fp64 reference for a non-zero, sign-mixed g0.  That pins the indexing: row maps, leading dimensions,
the [B,Hkv,S,G,D] / [B,Hkv,S,D] layouts, which row's rstd is used, every partial row counted exactly once, the
ping-pong between `partial` and its scratch across folds.

Every test also pins: inputs past rows / cols hold NaN, the elements after grad and after the partial buffer's
stated size hold canaries that come back unchanged, and a second call gives bit-identical outputs."""
import pytest
import torch

from tests import norm_util as U

pytestmark = pytest.mark.gpu

IDENT = (0, 0, 0, 0)
RSTDS = torch.tensor([1.0, 0.5, 0.25, 0.125])


def L():
    from projectiontrainer_amd import _lib
    return _lib


def finish_grad(g0, S):
    """bf16(g0 + bf16(S)) for an exactly summed S (fp64 holding an fp32-exact value)."""
    return (g0.float() + S.float().bfloat16().float()).bfloat16()


def with_canary(vals, n_extra=8):
    """bf16 [n + n_extra] on the CPU: vals then canaries."""
    out = torch.empty(vals.numel() + n_extra, dtype=torch.bfloat16)
    out[:vals.numel()] = vals
    U.bits(out)[vals.numel():] = U.CANARY_BITS
    return out


def check_grad(got, want, cols, what):
    got, want = got.cpu(), want.cpu()
    bad = (U.bits(got[:cols]) != U.bits(want[:cols])).nonzero().flatten().tolist()
    assert not bad, f"{what}: {len(bad)} of {cols} columns differ, first {bad[:8]}: " \
                    f"got {got[bad[:4]].tolist()} want {want[bad[:4]].tolist()}"
    assert bool((U.bits(got[cols:]) == U.CANARY_BITS).all()), f"{what}: wrote past cols"


# ---------------------------------------------------------------- rms_wgrad
# (rows, cols, pair, map kind): every rows value (1, 31, 32, 33: the 32-row block edge; 130: 5 blocks; 8225: 258 blocks,
# one colsum16 fold + finish16) and every cols value (4: one thread; 1020 / 1024 / 1028: the first column group's edge;
# the models' 1152 / 2560; 4096: the limit) appears, each pair three times, each map three times
RMS_CASES = [
    (1, 4, "ff", "ident"), (31, 1020, "bf", "offset"), (32, 1024, "fb", "grouped"), (33, 1028, "ff", "grouped"),
    (130, 1152, "bf", "ident"), (130, 2560, "fb", "offset"), (33, 4096, "ff", "offset"),
    (8225, 1028, "bf", "grouped"), (8225, 4, "fb", "ident"),
]


def make_map(kind, rows):
    """(map, number of x rows): an offset map, and a grouped map (groups of 5 rows, 9 apart, from row 2)."""
    if kind == "ident":
        return IDENT, rows
    if kind == "offset":
        return (0, 0, 0, 7), rows + 7
    g, gs, off = 5, 9, 2
    return (g, 0, gs, off), ((rows - 1) // g) * gs + (rows - 1) % g + off + 1


@pytest.mark.parametrize("rows,cols,pair,mapkind", RMS_CASES)
def test_rms_wgrad_exact(gpu, rows, cols, pair, mapkind):
    """pair: x / dy types -- ff: f32 / f32 with dy_round, bf: bf16 / f32 with dy_round, fb: f32 / bf16.  dy = k * 2^-8
    with |k| <= 300: bf16 keeps 8 significant bits, so dy_round changes every |k| > 256 that is odd (and the reference
    applies it); rounding after the product instead, or not at all, changes the sum.  unit = 2^-8 * 2^-3."""
    lib = L().lib()
    gen = torch.Generator().manual_seed(rows * 4099 + cols)
    m, xrows = make_map(mapkind, rows)
    src = U.map_rows(m, rows)
    ldx, lddy = cols + 8, cols + 4
    x = torch.randint(-2, 3, (rows, cols), generator=gen).double()
    dy = torch.randint(-300, 301, (rows, cols), generator=gen).double() * 2.0 ** -8
    rstd = RSTDS[torch.randint(0, 4, (rows,), generator=gen)].double()
    x_bf16, dy_bf16 = pair[0] == "b", pair[1] == "b"
    if dy_bf16:
        dy = U.bfr(dy)
    dy_used = dy if dy_bf16 else U.bfr(dy)
    if not dy_bf16:
        assert int((dy_used != dy).sum()) > 0 or rows * cols < 64     # dy_round has something to change
    terms = dy_used * x * rstd.unsqueeze(1)
    unit = 2.0 ** -11
    assert float(terms.abs().sum(dim=0).max()) < 2 ** 24 * unit
    assert bool((terms / unit == (terms / unit).round()).all())
    S = terms.sum(dim=0)
    g0 = U.nonzero_g0(cols, gen, scale=0.25)
    want = finish_grad(g0, S)

    xb = torch.full((xrows + 3, ldx), float("nan"), dtype=torch.float64)
    xb[src, :cols] = x
    xb = xb.to(torch.bfloat16 if x_bf16 else torch.float32).to(gpu)
    dyb = U.padded(dy, ld=lddy).to(torch.bfloat16 if dy_bf16 else torch.float32).to(gpu)
    rs = U.padded(rstd.float().unsqueeze(1)).flatten().to(gpu)
    need = lib.ptk_rms_wgrad_partial_floats(rows, cols)
    nblk = (rows + 31) // 32
    assert need == (nblk + (nblk + 15) // 16) * cols
    outs = []
    for _ in range(2):
        grad = with_canary(g0).to(gpu)
        part = torch.full((need + 64,), U.CANARY_F32, device=gpu)
        rc = lib.ptk_rms_wgrad(xb.data_ptr(), int(x_bf16), ldx, L().RowMap(*m), rs.data_ptr(), dyb.data_ptr(),
                               int(dy_bf16), lddy, 0 if dy_bf16 else 1, rows, cols, grad.data_ptr(), part.data_ptr(),
                               need, L().stream_ptr(gpu))
        assert rc == 0, lib.ptk_last_error()
        torch.cuda.synchronize()
        check_grad(grad, with_canary(want), cols, f"rms_wgrad {pair}")
        assert bool((part[need:] == U.CANARY_F32).all()), "wrote past the stated partial size"
        outs.append(grad.cpu())
    assert torch.equal(U.bits(outs[0]), U.bits(outs[1]))


def test_rms_wgrad_rejects_other_pairs_and_short_partials(gpu):
    """Host-side refusals with real device buffers: nothing is written."""
    lib = L().lib()
    x = torch.zeros(4, 8, device=gpu)
    grad = with_canary(torch.ones(8).bfloat16()).to(gpu)
    keep = grad.clone()
    part = torch.zeros(64, device=gpu)
    args = lambda xb, db, rnd, pf: (x.data_ptr(), xb, 8, L().RowMap(*IDENT), x.data_ptr(), x.data_ptr(), db, 8, rnd, 4,
                                    8, grad.data_ptr(), part.data_ptr(), pf, L().stream_ptr(gpu))
    assert lib.ptk_rms_wgrad(*args(1, 1, 0, 64)) == -1 and b"bf16" in lib.ptk_last_error()
    assert lib.ptk_rms_wgrad(*args(0, 0, 1, lib.ptk_rms_wgrad_partial_floats(4, 8) - 1)) == -1
    assert b"partial" in lib.ptk_last_error()
    torch.cuda.synchronize()
    assert torch.equal(U.bits(grad), U.bits(keep))


# ---------------------------------------------------------------- rms_wgrad_finish
# nblk: 1; 15 / 16 / 17 (one row group of finish16 full); 255 / 256 / 257 (finish16 alone up to 256, then one colsum16
# fold); 272 = 17 * 16; 4096 (one fold to 256); 4097 (two folds: partial -> scratch -> partial's head)
FINISH_CASES = [(1, 64), (15, 100), (16, 256), (17, 1152), (255, 100), (256, 64), (257, 1152), (272, 256),
                (4096, 100), (4097, 64), (4097, 1152)]


@pytest.mark.parametrize("nblk,cols", FINISH_CASES)
def test_rms_wgrad_finish_exact(gpu, nblk, cols):
    """Integer partials in [-8, 8] (unit 1): any order sums them exactly; the scratch rows behind them hold NaN."""
    lib = L().lib()
    gen = torch.Generator().manual_seed(nblk * 131 + cols)
    p = torch.randint(-8, 9, (nblk, cols), generator=gen).double()
    assert float(p.abs().sum(dim=0).max()) < 2 ** 24
    S = p.sum(dim=0)
    g0 = U.nonzero_g0(cols, gen)
    want = finish_grad(g0, S)
    need = lib.ptk_rms_wgrad_finish_floats(nblk, cols)
    assert need == (nblk + (nblk + 15) // 16) * cols
    outs = []
    for _ in range(2):
        buf = torch.full((need + 64,), float("nan"))
        buf[:nblk * cols] = p.float().flatten()
        buf[need:] = U.CANARY_F32
        buf = buf.to(gpu)
        grad = with_canary(g0).to(gpu)
        rc = lib.ptk_rms_wgrad_finish(buf.data_ptr(), nblk, cols, grad.data_ptr(), need, L().stream_ptr(gpu))
        assert rc == 0, lib.ptk_last_error()
        torch.cuda.synchronize()
        check_grad(grad, with_canary(want), cols, "rms_wgrad_finish")
        assert bool((buf[need:] == U.CANARY_F32).all()), "wrote past the stated partial size"
        outs.append(grad.cpu())
    assert torch.equal(U.bits(outs[0]), U.bits(outs[1]))


# ---------------------------------------------------------------- qknorm_wgrad
# (B, S, Hq, Hkv, D): D = 256 runs the one-wave-per-token kernel, the others the generic one; 3 x 37 = 111 token rows
# are no multiple of the 8-row block and positions restart per sample; 2 x 1030 rows give 258 blocks (a colsum16 fold)
QK_CASES = [(3, 37, 4, 1, 256), (3, 37, 8, 4, 256), (3, 37, 8, 4, 64), (3, 37, 2, 1, 8), (3, 37, 4, 1, 64),
            (2, 1030, 2, 1, 256), (2, 1030, 2, 1, 64)]


def qk_reference(qkv, cos, sin, rq, rk, dQ, dK, B, S, Hq, Hkv, D):
    """fp64 (sum_q, sum_k, largest sum of magnitudes): dn = RoPE^T(dr) = dr[d] c + dr[d + h] s (d < h),
    dr[d] c - dr[d - h] s (d >= h) with the tables' row `pos`; dw[d] = sum dn[d] x[d] rstd."""
    h, G = D // 2, Hq // Hkv
    x = qkv.view(B, S, Hq + 2 * Hkv, D)
    c, s = cos.view(1, S, 1, h), sin.view(1, S, 1, h)

    def one(dr, xh, rs):
        lo, hi = dr[..., :h], dr[..., h:]
        dn = torch.cat([lo * c + hi * s, hi * c - lo * s], dim=-1)
        mag = torch.cat([(lo * c).abs() + (hi * s).abs(), (hi * c).abs() + (lo * s).abs()], dim=-1)
        t = dn * xh * rs.unsqueeze(-1)
        return t.sum(dim=(0, 1, 2)), float((mag * xh.abs() * rs.unsqueeze(-1)).sum(dim=(0, 1, 2)).max())

    dq = dQ.view(B, Hkv, S, G, D).permute(0, 2, 1, 3, 4).reshape(B, S, Hq, D)      # head hq = kvh * G + j
    dk = dK.view(B, Hkv, S, D).permute(0, 2, 1, 3)
    sq, mq = one(dq, x[:, :, :Hq], rq.view(B, S, Hq))
    sk, mk = one(dk, x[:, :, Hq:Hq + Hkv], rk.view(B, S, Hkv))
    return sq, sk, max(mq, mk)


@pytest.mark.parametrize("B,S,Hq,Hkv,D", QK_CASES)
def test_qknorm_wgrad_exact(gpu, B, S, Hq, Hkv, D):
    """qkv, dQ, dK integers in [-3, 3], cos / sin in {-1, 0, 1/2, 1}, rstd in {1 .. 1/8}: unit 2^-4.  The v columns of
    qkv and table rows from S on (what a row index used as a position would read) hold NaN."""
    lib = L().lib()
    gen = torch.Generator().manual_seed(B * 1009 + S * 31 + Hq * 7 + D)
    M, h, G = B * S, D // 2, Hq // Hkv
    ri = lambda *shape: torch.randint(-3, 4, shape, generator=gen).double()
    qkv = ri(M, (Hq + 2 * Hkv) * D)
    dQ, dK = ri(B, Hkv, S, G, D), ri(B, Hkv, S, D)
    tab = torch.tensor([-1.0, 0.0, 0.5, 1.0], dtype=torch.float64)
    cos = tab[torch.randint(0, 4, (S, h), generator=gen)]
    sin = tab[torch.randint(0, 4, (S, h), generator=gen)]
    rq = RSTDS[torch.randint(0, 4, (M, Hq), generator=gen)].double()
    rk = RSTDS[torch.randint(0, 4, (M, Hkv), generator=gen)].double()
    sq, sk, mag = qk_reference(qkv, cos, sin, rq, rk, dQ, dK, B, S, Hq, Hkv, D)
    unit = 2.0 ** -4
    assert mag < 2 ** 24 * unit
    assert bool((sq / unit == (sq / unit).round()).all())
    g0q, g0k = U.nonzero_g0(D, gen), U.nonzero_g0(D, gen)
    want_q, want_k = finish_grad(g0q, sq), finish_grad(g0k, sk)

    qkv_d = qkv.clone()
    qkv_d[:, (Hq + Hkv) * D:] = float("nan")
    qkv_d = qkv_d.bfloat16().to(gpu)
    pad_tab = lambda t: torch.cat([t, torch.full((M - S, h), float("nan"), dtype=t.dtype)]).float().to(gpu)
    cos_d, sin_d = pad_tab(cos), pad_tab(sin)
    dQ_d, dK_d = dQ.bfloat16().to(gpu), dK.bfloat16().to(gpu)
    rq_d, rk_d = rq.float().to(gpu), rk.float().to(gpu)
    need = lib.ptk_qknorm_wgrad_partial_floats(M, D)
    nblk = (M + 7) // 8
    assert need == (2 * nblk + (nblk + 15) // 16) * D
    outs = []
    for _ in range(2):
        gq, gk = with_canary(g0q).to(gpu), with_canary(g0k).to(gpu)
        part = torch.full((need + 64,), U.CANARY_F32, device=gpu)
        rc = lib.ptk_qknorm_wgrad(qkv_d.data_ptr(), cos_d.data_ptr(), sin_d.data_ptr(), B, S, Hq, Hkv, D,
                                  rq_d.data_ptr(), rk_d.data_ptr(), dQ_d.data_ptr(), dK_d.data_ptr(), gq.data_ptr(),
                                  gk.data_ptr(), part.data_ptr(), need, L().stream_ptr(gpu))
        assert rc == 0, lib.ptk_last_error()
        torch.cuda.synchronize()
        check_grad(gq, with_canary(want_q), D, "q_norm grad")
        check_grad(gk, with_canary(want_k), D, "k_norm grad")
        assert bool((part[need:] == U.CANARY_F32).all()), "wrote past the stated partial size"
        outs.append((gq.cpu(), gk.cpu()))
    assert torch.equal(U.bits(outs[0][0]), U.bits(outs[1][0])) and torch.equal(U.bits(outs[0][1]), U.bits(outs[1][1]))
