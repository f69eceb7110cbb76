"""The loss head of ptk_gemma3_*_fwd_bwd kernel by kernel, through its test-facing entries, against plain fp64 on the
CPU (tests/loss_util.py): the lm_head GEMM's softmax-statistics epilogue on the three tile families that carry it
(gemm.hip epilogue<ACT_NONE, OUT_BF16> under the 128x128, the 256x256 and the staggered 256x256 kernel),
ce_stats_kernel, the two-pass ce_kernel, ce_write_dlogits, count_valid_kernel and loss_reduce_kernel (misc.hip).

Every comparison is with fp64 evaluated on the bf16 values the kernel itself stored, never with another kernel.

Operands.  tests/loss_util.py exact_operands: multiples of 1/8 in [-2, 2], K 64 or 128, so every fp32 partial sum is
exact and the logits must equal bf16_rne(A . B^T) bit for bit on every family.  A few rows of A are scaled by 8
(|logit| in the hundreds: no max subtraction, no finite result) and a few by 1/8 (crowded rows with ties).

Bars.
  logits      bit equality.
  chunk max   bit equality with the maximum of the stored bf16 values.
  chunk sum   loss_util.chunk_sum_bound, derived per chunk from the data (argument roundings of the exp2, 2^-21
              relative for the hardware exp2 and the 6 additions a term passes through).  The 2^-21 is relative to
              the sum: as an absolute term it would lie below half an fp32 ulp of any sum above 4, which no stored
              fp32 sum of a crowded chunk could meet.
  row_loss    the yardstick is torch's own fp32 F.cross_entropy(reduction='none') on the same stored logits against
              the same fp64 value, taken relative to the row's scale s = max(|lse|, |x_target|) (the magnitude whose
              fp32 spacing bounds both lse = M + log S and lse - x_target) and maximised over the case's valid rows:
              y = max_r |torch32_r - ref_r| / s_r.  A kernel row may miss fp64 by (4 y + 2 eps32) s_r, and the two
              entries may differ from each other by as much.  Ignored rows are exactly 0.
  d(logits)   every element |got - exact| <= ulp_bf16(exact) / 2 + 1e-5 g (p + [c == target]); a 0 is accepted
              where |exact| is below the fp32 normal range; ignored rows are exactly 0 in every column.

Shapes are the smallest that reach each branch: M 1 .. 300 crosses the epilogue's 64-row block, the 128- and 256-row
tiles and the top / bot halves of a 256x256 wave; V 64 .. 32832 gives fewer chunks than threads, exactly 256, 289 and
513 chunks in ce_stats_kernel, a tail-only ce_write_dlogits (V <= 14336), its 8-deep group loop alone (16384) and
with a tail behind it (18496, 32832); V 8, 2056, 14344 (V % 64 != 0) exist on the two-pass kernel only.  Leading dimensions with and
without slack; every buffer is pre-filled with poison, which rows >= M, columns >= V and the slack must keep.
No input makes a kernel read or write out of bounds: targets are -100 or in [0, V), leading dimensions validated.

Measured on an MI355X (the largest over all cases; each test prints its own figures before it asserts):
  chunk-sum error / bound                   0.948  (the same on all three tile families).  The worst chunk is one of
                                            a row scaled by 8: maximum 360, every other term underflows, sum 1.  Its
                                            bound is almost all one rounding, fl(-m L2E) at ulp32 2^-14, and that
                                            rounding alone comes to 0.947 of it for m = 360 (computed on the CPU)
  row_loss yardstick y (torch fp32)         9.2e-8   (so a row may be off by at most 4.8e-7 s)
  row_loss |err| / s, statistics entry      9.2e-8   (0.19 of the allowed)
  row_loss |err| / s, two-pass entry        1.04e-7  (0.22 of the allowed)
  row_loss |statistics - two-pass| / s      1.36e-7
  hand-built statistics, |err| / s          3.1e-8   (yardstick 3.1e-8)

Mutations, each applied alone to a scratch copy of the library, this file run once against it (70 tests):
  1. statistics epilogue, final max select swapped (b3 ? m2[0] : m2[1]): 48 failed, every test_gemm_row_stats and
     test_lm_head_then_cross_entropy case ("a chunk max is not the max of the stored logits")
  2. ce_write_dlogits' tail loop comparing with tgt + 1: 34 failed, test_lm_head_then_cross_entropy at every V but
     16384 (whose rows end inside the group loop), every test_two_pass_cross_entropy_ragged_vocab case and both
     test_cross_entropy_stats_hand_built cases (d(logits) outside the bound at the target column)
  3. ce_stats_kernel without the s * exp(m - mn) rescale: 9 failed, test_lm_head_then_cross_entropy at V 18496 and
     32832 (the vocabularies where a thread owns more than one chunk) and test_cross_entropy_stats_hand_built[18496]
     (row_loss off by 1e-2 s against an allowed 5e-7 s)"""
import functools
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import loss_util as U

pytestmark = pytest.mark.gpu

MS = (1, 7, 63, 64, 65, 127, 129, 255, 257, 300)
MODES = {1: "nt128", 2: "big", 4: "big2"}            # ptk_gemm_force_small_tiles mode -> ptk_gemm_path_counts family
ROWS = 300
BIG_ROWS, SMALL_ROWS = (3, 66, 130, 258, 299), (5, 64, 128, 200, 256)
PAD = 3


def _k():
    from projectiontrainer_amd import _lib as L
    from projectiontrainer_amd import kernels as Kn
    return Kn, L


def kdepth(N):
    return 64 if N in (64, 2112, 18496, 8, 14344) else 128


def note(name, **figs):
    print("LOSSHEAD " + name + " " + " ".join(f"{k}={v:.4g}" for k, v in figs.items()))


# ---------------------------------------------------------------- shared references (computed once, never written)
@functools.lru_cache(maxsize=None)
def gemm_ref(N):
    K = kdepth(N)
    A, B = U.exact_operands(ROWS, N, K, seed=100 + N, big_rows=BIG_ROWS, small_rows=SMALL_ROWS)
    _, L16 = U.exact_logits(A, B)
    mx, sm = U.chunk_stats_ref(L16)
    return types.SimpleNamespace(A=A, B=B, L16=L16, mx=mx, sm=sm, bound=U.chunk_sum_bound(L16))


def targets_for(R, V, seed):
    """0, V - 1, 63, 64 (where the vocabulary has them) in rows 0 .. 3, ignored rows at 4, in the middle and last, and
    one target per further row elsewhere."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, V, (R,), generator=g)
    t[0], t[1], t[2], t[3] = 0, V - 1, min(63, V - 1), min(64, V - 1)
    t[4] = t[R // 2] = t[R - 1] = U.IGNORE
    return t


CE_ROWS = 24
CE_BIG, CE_SMALL = (5, 6, 12, 20), (7, 8, 21, 23)        # (12 and 23 are ignored rows: scaled rows among them too)


@functools.lru_cache(maxsize=None)
def ce_ref(V):
    K = kdepth(V)
    A, B = U.exact_operands(CE_ROWS, V, K, seed=900 + V, big_rows=CE_BIG, small_rows=CE_SMALL)
    _, L16 = U.exact_logits(A, B)
    tgt = targets_for(CE_ROWS, V, seed=V)
    stats = {}
    if V % 64 == 0:
        mx, sm = U.chunk_stats_ref(L16)
        stats = dict(mx=mx, sm=sm, bound=U.chunk_sum_bound(L16))
    return types.SimpleNamespace(A=A, B=B, L16=L16, tgt=tgt, **stats, **loss_refs(L16, tgt))


def loss_refs(L16, tgt):
    """fp64 loss, the rows' scale s and torch's fp32 yardstick y for bf16 logits."""
    lse = U.lse_ref(L16)
    loss = U.row_loss_ref(L16, tgt)
    valid = tgt >= 0
    xt = L16.double().gather(1, tgt.clamp(min=0).unsqueeze(1)).squeeze(1)
    scale = torch.maximum(lse.abs(), xt.abs())
    t32 = F.cross_entropy(L16.float(), tgt, reduction="none", ignore_index=U.IGNORE).double()
    finite = valid & torch.isfinite(loss)
    yard = float(((t32 - loss).abs() / scale)[finite].max())
    return dict(lse=lse, loss=loss, valid=valid, scale=scale, yard=yard)


# ---------------------------------------------------------------- checks
def poisoned_logits(rows, ld, gpu, L16=None):
    buf = U.poison_bf16(rows + PAD, ld)
    if L16 is not None:
        buf[:L16.shape[0], :L16.shape[1]] = L16
    return buf.to(gpu)


def logits_poison_intact(c, rows, V):
    b = U.bits(c)
    return bool((b[rows:] == U.POISON_BF16).all()) and bool((b[:, V:] == U.POISON_BF16).all())


def check_row_loss(name, rl, ref, rows=None):
    """rl (f32 [R], from the device) against fp64 at (4 y + 2 eps32) s per row; ignored rows exactly 0."""
    rl = rl.cpu().double()
    keep = ref.valid if rows is None else ref.valid & rows
    err = ((rl - ref.loss).abs() / ref.scale)[keep]
    allowed = 4 * ref.yard + 2 * U.EPS32
    note(name, yard=ref.yard, err=float(err.max()), ratio=float(err.max()) / allowed)
    assert bool((err <= allowed).all()), f"{name}: row_loss off by {float(err.max()):.3e} s, allowed {allowed:.3e} s"
    assert not rl[~ref.valid].any(), f"{name}: an ignored row has a loss"


def check_dlogits(name, got, L16, tgt, g, rows=None):
    R, V = L16.shape
    got = got.cpu()[:R, :V]
    exact, weight = U.dlogits_ref(L16, tgt, g)
    ok = U.dlogits_ok(got, exact, weight, g)
    if rows is not None:
        ok = ok | ~rows.unsqueeze(-1)
    bad = (~ok).nonzero()
    assert bad.numel() == 0, f"{name}: {bad.shape[0]} of {ok.numel()} d(logits) outside the bound, first (row, col) " \
                             f"{bad[0].tolist()}: got {float(got[tuple(bad[0])]):.6e} exact {float(exact[tuple(bad[0])]):.6e}"
    ign = got[tgt < 0].float()
    assert not ign.any(), f"{name}: an ignored row has a gradient"


def run_gemm_stats(A, B, M, N, ldc, lds, mode, gpu):
    Kn, L = _k()
    C = poisoned_logits(M, ldc, gpu)
    S = torch.full((M + PAD, lds), U.POISON_F32).to(gpu)
    L.check(L.lib().ptk_gemm_force_small_tiles(mode), "force")
    L.gemm_path_counts(reset=True)
    try:
        Kn.gemm_row_stats(A[:M], B, C, S, M=M, N=N, ldc=ldc, ld_stats=lds)
        paths = L.gemm_path_counts(reset=True)
    finally:
        L.lib().ptk_gemm_force_small_tiles(0)
    return C, S, paths


def check_gemm_stats(name, c, s, ref, M, N):
    """logits bit-exact, chunk max bit-exact, chunk sum inside the derived bound, poison kept.  Returns the largest
    sum error / bound."""
    nch = N // 64
    assert torch.equal(U.bits(c[:M, :N]), U.bits(ref.L16[:M])), f"{name}: logits differ from bf16_rne(A . B^T)"
    assert logits_poison_intact(c, M, N), f"{name}: logits written past row M or column N"
    st = s[:M, :2 * nch].reshape(M, nch, 2)
    assert torch.equal(st[..., 0].contiguous().view(torch.int32), ref.mx[:M].float().view(torch.int32)), \
        f"{name}: a chunk max is not the max of the stored logits"
    ratio = (st[..., 1].double() - ref.sm[:M]).abs() / ref.bound[:M]
    worst = float(ratio.max())
    assert not torch.isnan(ratio).any() and worst <= 1.0, \
        f"{name}: chunk sum error / bound {worst:.3f} at (row, chunk) {np.unravel_index(int(ratio.nan_to_num(9e9).argmax()), ratio.shape)}"
    assert bool((s[M:] == U.POISON_F32).all()), f"{name}: statistics written at rows >= M"
    assert bool((s[:, 2 * nch:] == U.POISON_F32).all()), f"{name}: statistics written into the slack of ld_stats"
    return worst


# ---------------------------------------------------------------- 1-3: the statistics epilogue
# every mode takes every shape here (K 64 is one K-tile, which all three kernels' prologues handle; rows and columns
# past M / N are clamped on the load side), so no (mode, shape) pair is dropped
@pytest.mark.parametrize("slack", [False, True], ids=["packed", "slack"])
@pytest.mark.parametrize("N,ms", [(64, MS), (192, MS), (2112, MS), (18496, (129, 257))],
                         ids=["N64", "N192", "N2112", "N18496"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_gemm_row_stats(gpu, mode, N, ms, slack):
    Kn, L = _k()
    ref = gemm_ref(N)
    A, B = ref.A.to(gpu), ref.B.to(gpu)
    ldc, lds = N + (8 if slack else 0), 2 * (N // 64) + (2 if slack else 0)
    worst = 0.0
    for M in ms:
        C, S, paths = run_gemm_stats(A, B, M, N, ldc, lds, mode, gpu)
        assert paths == {(MODES[mode], L.ACT_NONE): 1}, (M, paths)
        worst = max(worst, check_gemm_stats(f"mode {mode} M {M} N {N}", C.cpu(), S.cpu(), ref, M, N))
    note(f"gemm_row_stats mode={mode} N={N}", chunk_ratio=worst)


# ---------------------------------------------------------------- 4-5: both CE entries from the GEMM's own output
def gscale_for(kind, tgt, gpu):
    """(device gscale [1], its value) for g = 1 or 0.25 / count, the latter from ptk_count_valid itself."""
    Kn, _ = _k()
    if kind == "one":
        return torch.ones(1, device=gpu), 1.0
    gs, cnt = Kn.count_valid(tgt.to(gpu), 0.25)
    n = int((tgt != U.IGNORE).sum())
    assert float(cnt.cpu()) == n
    want = np.float32(0.25) / np.float32(n)
    assert np.float32(gs.cpu().numpy()[0]) == want
    return gs, float(want)


@pytest.mark.parametrize("gkind", ["one", "count"])
@pytest.mark.parametrize("slack", [False, True], ids=["packed", "slack"])
@pytest.mark.parametrize("V", [64, 192, 2112, 16384, 18496, 32832])
def test_lm_head_then_cross_entropy(gpu, V, slack, gkind):
    """ptk_gemm_row_stats -> ptk_cross_entropy_stats, and ptk_cross_entropy on a copy of the same logits."""
    Kn, L = _k()
    ref = ce_ref(V)
    R = CE_ROWS
    ld, lds = V + (8 if slack else 0), 2 * (V // 64) + (2 if slack else 0)
    C, S, paths = run_gemm_stats(ref.A.to(gpu), ref.B.to(gpu), R, V, ld, lds, 0, gpu)
    assert paths == {("nt128", L.ACT_NONE): 1}, paths
    note(f"lm_head V={V}", chunk_ratio=check_gemm_stats(f"lm_head V {V}", C.cpu(), S.cpu(), ref, R, V))
    tgt = ref.tgt.to(gpu)
    gs, g = gscale_for(gkind, ref.tgt, gpu)
    c1, c2 = C.clone(), C.clone()
    rl1 = Kn.cross_entropy_stats_(c1[:R], S[:R], tgt, gs, vocab=V)
    rl2 = Kn.cross_entropy_(c2[:R, :V], tgt, gs)
    check_row_loss(f"stats V={V}", rl1, ref)
    check_row_loss(f"two-pass V={V}", rl2, ref)
    diff = ((rl1.cpu().double() - rl2.cpu().double()).abs() / ref.scale)[ref.valid]
    note(f"agree V={V}", err=float(diff.max()))
    assert bool((diff <= 4 * ref.yard + 2 * U.EPS32).all()), "the two entries disagree"
    for name, c in (("stats", c1), ("two-pass", c2)):
        c = c.cpu()
        assert logits_poison_intact(c, R, V), f"{name}: d(logits) written past row R or column V"
        check_dlogits(f"{name} V={V} g={g:.4g}", c, ref.L16, ref.tgt, g)
    assert torch.equal(S.cpu()[R:], torch.full((PAD, lds), U.POISON_F32))


@pytest.mark.parametrize("gkind", ["one", "count"])
@pytest.mark.parametrize("slack", [False, True], ids=["packed", "slack"])
@pytest.mark.parametrize("V", [8, 2056, 14344])
def test_two_pass_cross_entropy_ragged_vocab(gpu, V, slack, gkind):
    """V % 64 != 0: the vocabularies only ce_kernel takes."""
    Kn, _ = _k()
    ref = ce_ref(V)
    R, ld = CE_ROWS, V + (8 if slack else 0)
    c = poisoned_logits(R, ld, gpu, ref.L16)
    gs, g = gscale_for(gkind, ref.tgt, gpu)
    rl = Kn.cross_entropy_(c[:R, :V], ref.tgt.to(gpu), gs)
    check_row_loss(f"two-pass V={V}", rl, ref)
    c = c.cpu()
    assert logits_poison_intact(c, R, V)
    check_dlogits(f"two-pass V={V} g={g:.4g}", c, ref.L16, ref.tgt, g)


# ---------------------------------------------------------------- 6: hand-built statistics
@pytest.mark.parametrize("V", [192, 18496])
def test_cross_entropy_stats_hand_built(gpu, V):
    """An all -inf chunk with statistics (-inf, NaN) leaves its row finite and right; the row maximum in the first
    and in the last chunk (at 289 chunks a thread's second chunk: both rescale directions); a NaN chunk max makes
    that row's loss NaN and no other's."""
    Kn, _ = _k()
    R, nch = 6, V // 64
    gen = torch.Generator().manual_seed(V)
    L16 = (torch.randn(R, V, generator=gen) * 3).bfloat16()
    L16[0, 64:128] = float("-inf")
    L16[1, 5] = 40.0
    L16[2, V - 3] = 40.0
    tgt = torch.tensor([3, 5, V - 3, 130, U.IGNORE, V - 1])
    mx, sm = U.chunk_stats_ref(L16)
    assert mx[0, 1] == float("-inf") and torch.isnan(sm[0, 1])
    lds = 2 * nch + 2
    S = torch.full((R + PAD, lds), U.POISON_F32)
    S[:R, 0:2 * nch:2], S[:R, 1:2 * nch:2] = mx.float(), sm.float()
    S[3, 2 * (nch - 1)] = float("nan")
    ref = types.SimpleNamespace(**loss_refs(L16, tgt))
    assert torch.isfinite(ref.loss).all()
    c = poisoned_logits(R, V + 8, gpu, L16)
    rl = Kn.cross_entropy_stats_(c[:R], S.to(gpu)[:R], tgt.to(gpu), torch.ones(1, device=gpu), vocab=V)
    got = rl.cpu()
    assert torch.isnan(got[3]), "a NaN chunk max must make the row's loss NaN"
    others = torch.tensor([True, True, True, False, True, True])
    assert torch.isfinite(got[others]).all()
    check_row_loss(f"hand-built V={V}", rl, ref, rows=others)
    c = c.cpu()
    assert logits_poison_intact(c, R, V)
    check_dlogits(f"hand-built V={V}", c, L16, tgt, 1.0, rows=others)
    assert not c[0, 64:128].float().any()                  # exp(-inf - lse) g: exactly 0


# ---------------------------------------------------------------- 7-8: the two reductions
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_count_valid(gpu, n):
    Kn, L = _k()
    gen = torch.Generator().manual_seed(n)
    cases = []
    for first, last in ((False, False), (True, False), (False, True), (True, True)):
        lab = torch.randint(0, 1000, (n,), generator=gen)
        lab[torch.rand(n, generator=gen) < 0.3] = U.IGNORE
        lab[0] = U.IGNORE if first else 7
        lab[n - 1] = U.IGNORE if last else (lab[n - 1] if n == 1 else 9)
        cases.append(lab)
    cases.append(torch.full((n,), U.IGNORE))
    for lab in cases:
        for scale in (1.0, 0.25, 1.0 / 3.0):
            gs, cnt = Kn.count_valid(lab.to(gpu), scale)
            want = int((lab != U.IGNORE).sum())
            assert float(cnt.cpu()) == want
            g = np.float32(gs.cpu().numpy()[0])
            assert g == (np.float32(scale) / np.float32(want) if want else np.float32(0)), (n, want, scale, g)
    # n = 0: nothing counted, both outputs written
    gs = torch.full((1,), U.POISON_F32, device=gpu)
    cnt = torch.full((1,), U.POISON_F32, device=gpu)
    L.check(L.lib().ptk_count_valid(None, 0, 1.0, L.ptr(gs), L.ptr(cnt), L.stream_ptr(gpu)), "count_valid")
    assert float(gs.cpu()) == 0 and float(cnt.cpu()) == 0


@pytest.mark.parametrize("rows", [1, 257, 1000])
def test_loss_reduce(gpu, rows):
    Kn, L = _k()
    gen = torch.Generator().manual_seed(rows)
    rl = torch.rand(rows, generator=gen) * 12
    rl[torch.rand(rows, generator=gen) < 0.25] = 0.0
    for count in (float(max(1, int((rl != 0).sum()))), 3.0):
        got = Kn.loss_reduce(rl.to(gpu), torch.tensor([count], device=gpu))
        want = rl.double().sum() / count
        torch.testing.assert_close(got.cpu().double()[0], want, rtol=1e-6, atol=0)
    assert torch.isnan(Kn.loss_reduce(rl.to(gpu), torch.zeros(1, device=gpu)).cpu()).all()
    # rows = 0: the empty sum over a positive count
    loss = torch.full((1,), U.POISON_F32, device=gpu)
    cnt = torch.tensor([4.0], device=gpu)
    L.check(L.lib().ptk_loss_reduce(None, 0, L.ptr(cnt), L.ptr(loss), L.stream_ptr(gpu)), "loss_reduce")
    assert float(loss.cpu()) == 0
