"""tests/gemm_ref.py checked without a GPU: the row map against a brute-force loop, the exactness claim of the dyadic
operands, the fp32 restatements of the transcendental epilogues against the cap, the reference itself on hand-made
descriptors, and the pinned dispatch table of the GPU cases (tests/data/gemm_contract_plan.json) with the coverage
it has to keep."""
import pytest
import torch

from tests import gemm_ref as G

MAPS = sorted({c["amap"] for c in G.CASES} | {c["cmap"] for c in G.CASES} | {G.ROUND2["cmap"], (7, 3, 5, -3)})


def test_map_row_against_a_loop():
    for g, skip, gs, off in MAPS:
        want = []
        for r in range(700):
            if g == 0:
                want.append(r + off if r + off >= 0 else -1)
            else:
                want.append(-1 if r % g < skip else (r // g) * gs + r % g + off)
        assert [G.map_row(g, skip, gs, off, r) for r in range(700)] == want, (g, skip, gs, off)
        assert G.map_rows((g, skip, gs, off), 700).tolist() == want, (g, skip, gs, off)
    assert G.map_row(0, 0, 0, -7, 6) == -1 and G.map_row(0, 0, 0, -7, 7) == 0
    assert G.map_row(60, 1, 80, -1, 60) == -1 and G.map_row(60, 1, 80, -1, 61) == 80
    assert G.map_row(75, 0, 96, 5, 149) == 96 + 74 + 5


def test_dyadic_products_are_exact_in_any_order():
    """fp32 A @ B.T equals the fp64 product bit for bit at the largest K, over three shuffled summation orders (and a
    one-term-at-a-time fp32 loop, the order least like a blocked matmul)."""
    K = max(c["K"] for c in G.CASES)
    assert K == 320 and all(c["K"] in (64, 128, 192, 320) for c in G.CASES)
    A, B = G.dyadic((96, K), -2, 2, 0, 1), G.dyadic((80, K), -4, 4, 6, 2)
    assert A.dtype == torch.bfloat16 and torch.equal(A.double(), G.dyadic((96, K), -2, 2, 0, 1, torch.float64))
    assert torch.equal(B.double(), G.dyadic((80, K), -4, 4, 6, 2, torch.float64))        # (bf16 holds them exactly)
    want = A.double() @ B.double().T
    assert float(want.abs().max()) < 64 and torch.equal(want * 64, (want * 64).round())
    for seed in range(3):
        p = torch.randperm(K, generator=torch.Generator().manual_seed(seed))
        got = A.float()[:, p] @ B.float()[:, p].T
        assert torch.equal(got.double(), want), seed
        acc = torch.zeros(96, 80)
        for k in p.tolist():
            acc += A.float()[:, k, None] * B.float()[None, :, k]
        assert torch.equal(acc.double(), want), seed
    # the additive inputs and alpha keep the sums exact: multiples of 2^-7 below 2^7
    v = 0.5 * want + G.dyadic((96, 80), -64, 64, 6, 3, torch.float64) + G.dyadic((96, 80), -64, 64, 6, 4, torch.float64)
    assert torch.equal(v.float().double(), v) and float(v.abs().max()) < 128


def _preacts():
    """The exact pre-activations of every transcendental GPU case (both M): {act: [fp64 tensors]} and, for the
    backward, (dh, saved pre-activation) pairs, from the very operands build() draws."""
    out = {a: [] for a in (G.ACT_GELU_TANH, G.ACT_GELU_ERF, G.ACT_GEGLU, G.ACT_GELU_ERF_BWD)}
    for c in G.CASES:
        if c["act"] not in out:
            continue
        for M in G.MS:
            b = G.build(c, M, "cpu")
            kw = dict(b.kw, act=G.ACT_NONE, out_mode=G.OUT_F32, cmap=(0, 0, 0, 0), aux=None, aux2=None)
            aux_in = kw.pop("aux_in", None)
            kw["C"] = torch.zeros(M, c["N"], dtype=torch.float32)
            pre = G.bfr(G.ref(b.A, b.B, **kw).exp["C"].double())      # steps 1-5: the bf16 pre-activation
            out[c["act"]].append((pre, aux_in[:M, :c["N"]].double()) if aux_in is not None else pre)
    return out


def test_fp32_restatements_stay_far_inside_the_cap():
    """On the exact inputs of the GPU cases, fp32 evaluation of the four forms differs from bf16(fp64 form) in at most
    1e-4 of the elements (20x inside NEQ_CAP), and the pre-activations have a standard deviation of at most ~1."""
    pre = _preacts()
    f32 = lambda x: x.to(torch.float32)
    bf = lambda x: x.to(torch.float32).to(torch.bfloat16)
    share = {}

    def tally(name, got, want):
        n, d = share.get(name, (0, 0))
        share[name] = (n + want.numel(), d + int((G.bits(bf(got)) != G.bits(bf(G.bfr(want)))).sum()))

    for x in pre[G.ACT_GELU_TANH]:
        assert float(x.std()) <= 1.1
        tally("tanh", G.f32_gelu_tanh(f32(x)), G.gelu_tanh(x))
    for x in pre[G.ACT_GELU_ERF]:
        assert float(x.std()) <= 1.1
        tally("erf", G.f32_gelu_erf(f32(x)), G.gelu_erf(x))
    for x in pre[G.ACT_GEGLU]:
        assert float(x.std()) <= 1.1
        M, N = x.shape
        x4 = x.reshape(M, N // 32, 2, 16)
        g, u = x4[:, :, 0, :], x4[:, :, 1, :]
        a32 = bf(G.f32_gelu_tanh(f32(g)))
        tally("geglu_a", a32, G.gelu_tanh(g))
        tally("geglu_b", G.f32_geglu_b(f32(g), f32(u)), G.gelu_tanh_grad(g) * u)
        tally("geglu_h", a32.float() * f32(u), G.bfr(G.gelu_tanh(g)) * u)
    for dh, x in pre[G.ACT_GELU_ERF_BWD]:
        assert float(x.std()) <= 1.1 and float(dh.std()) <= 1.1
        tally("erf_bwd", G.f32_gelu_erf_bwd(f32(dh), f32(x)), dh * G.gelu_erf_grad(x))
    assert set(share) == {"tanh", "erf", "geglu_a", "geglu_b", "geglu_h", "erf_bwd"}
    for name, (n, d) in share.items():
        assert n >= 2 ** 17 and d <= 1e-4 * n, (name, n, d)
    assert 1e-4 * 20 <= G.NEQ_CAP


def test_reference_on_hand_made_descriptors():
    """ref() on descriptors small enough to work out by hand: the order of the roundings, the unmapped aux row against
    the mapped C / resid row, the interleaved GEGLU columns, untouched rows."""
    bf16, f32 = torch.bfloat16, torch.float32
    A = torch.zeros(4, 64, dtype=bf16)
    A[:, 0] = torch.tensor([1.0, 2.0, 3.0, 4.0])
    B = torch.zeros(32, 64, dtype=bf16)
    B[:, 0] = 1.0                                              # A . B^T [r][c] = r + 1
    # bias 1/256 is lost by bf16_linear at 2, 3, 4 (8 significand bits) but not by a late rounding to f32
    bias = torch.full((32,), 2.0 ** -8, dtype=f32)
    C = G.guard_fill(torch.empty(12, 32, dtype=f32))
    resid = torch.full((12, 32), 100.0, dtype=f32)
    resid[9] = 200.0
    r = G.ref(A, B, C=C, M=4, N=32, K=64, bias=bias, bf16_linear=True, resid=resid, cmap=(2, 1, 8, 0), out_mode=G.OUT_F32)
    assert r.written["C"].nonzero()[:, 0].unique().tolist() == [1, 9]      # rows 0, 2 dropped; 1 -> 1, 3 -> 8 + 1
    assert torch.equal(r.exp["C"][1], torch.full((32,), 102.0)) and torch.equal(r.exp["C"][9], torch.full((32,), 204.0))
    assert G.guard_intact(r.exp["C"], r.written["C"]) == 0
    r = G.ref(A, B, C=C, M=4, N=32, K=64, bias=bias, out_mode=G.OUT_F32)
    assert torch.equal(r.exp["C"][:4, 0], torch.tensor([1.0, 2.0, 3.0, 4.0]) + 2.0 ** -8)
    r = G.ref(A, B, C=C, M=4, N=32, K=64, bias=bias, out_mode=G.OUT_F32_BF16ROUND, alpha=0.5)
    assert torch.equal(r.exp["C"][:4, 0], torch.tensor([0.5 + 2.0 ** -8, 1.0, 1.5, 2.0]))   # (ties to even)
    # GELU-erf: aux (the pre-activation) at the unmapped row, C at the mapped one
    Cb, aux = G.guard_fill(torch.empty(12, 32, dtype=bf16)), G.guard_fill(torch.empty(6, 40, dtype=bf16))
    r = G.ref(A, B, C=Cb, M=4, N=32, K=64, act=G.ACT_GELU_ERF, aux=aux, cmap=(0, 0, 0, 5))
    assert torch.equal(r.exp["aux"][:4, :32].float(), torch.tensor([1.0, 2.0, 3.0, 4.0])[:, None].expand(4, 32))
    assert r.written["aux"][:4, :32].all() and int(r.written["aux"].sum()) == 128
    want = torch.nn.functional.gelu(torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=torch.float64)).float().to(bf16)
    assert torch.equal(r.exp["C"][5:9, 7], want) and int(r.written["C"].sum()) == 128 and not r.exact
    # GEGLU: column 0 is gate, column 16 the up of h column 0
    B2 = torch.zeros(32, 64, dtype=bf16)
    B2[:16, 0], B2[16:, 0] = 0.5, 2.0
    Ch, a1, a2 = (G.guard_fill(torch.empty(4, 16, dtype=bf16)) for _ in range(3))
    r = G.ref(A, B2, C=Ch, M=4, N=32, K=64, act=G.ACT_GEGLU, aux=a1, aux2=a2)
    g = torch.tensor([0.5, 1.0, 1.5, 2.0], dtype=torch.float64)
    u = 4 * g
    fa = torch.nn.functional.gelu(g, approximate="tanh").float().to(bf16)
    assert torch.equal(r.exp["aux"][:, 3], fa) and torch.equal(r.exp["C"][:, 3], (fa.double() * u).float().to(bf16))
    gg = g.clone().requires_grad_(True)
    torch.nn.functional.gelu(gg, approximate="tanh").sum().backward()
    assert torch.equal(r.exp["aux2"][:, 15], (gg.grad * u).float().to(bf16))
    # GEGLU backward: dg | du interleaved in 16-column groups, exact
    fa_in, fb_in = torch.full((4, 32), 3.0, dtype=bf16), torch.full((4, 32), 5.0, dtype=bf16)
    Cg = G.guard_fill(torch.empty(4, 64, dtype=bf16))
    r = G.ref(A, B, C=Cg, M=4, N=32, K=64, act=G.ACT_GEGLU_BWD, aux_in=fa_in, aux_in2=fb_in)
    row = r.exp["C"][1].float()
    assert row[:16].eq(10).all() and row[16:32].eq(6).all() and row[32:48].eq(10).all() and row[48:].eq(6).all()
    assert r.exact
    # GELU-erf backward against autograd
    x_in = torch.linspace(-2, 2, 4 * 32).reshape(4, 32).to(bf16)
    r = G.ref(A, B, C=Cb, M=4, N=32, K=64, act=G.ACT_GELU_ERF_BWD, aux_in=x_in)
    xx = x_in.double().requires_grad_(True)
    torch.nn.functional.gelu(xx).sum().backward()
    assert torch.equal(r.exp["C"][:4], (torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=torch.float64)[:, None] * xx.grad).float().to(bf16))
    assert r.scale == 4.0


def test_bf16_rounding_of_fp64_is_single():
    """bfr rounds the fp64 value once: equal to torch's fp32 -> bf16 conversion wherever fp32 holds the value, ties
    to even, and not fooled by a value that fp32 would first round onto a tie."""
    x = (torch.randn(1 << 16, generator=torch.Generator().manual_seed(5)) * 3.0).double()    # fp32 values
    x = torch.cat([x, torch.tensor([0.0, 1.0, -1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(2.0 + 2.0 ** -7), 2.0 ** -100])])
    assert torch.equal(G.bfr(x), x.float().to(torch.bfloat16).double())
    assert G.bfr(torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], dtype=torch.float64)).tolist() == [1.0, 1.015625]
    y = torch.tensor([1.003906289545454, -2.007812579090908], dtype=torch.float64)           # 3.9e-8 past a tie
    assert G.bfr(y).tolist() == [1.0078125, -2.015625]
    assert y.float().to(torch.bfloat16).double().tolist() == [1.0, -2.0]                     # (the double rounding)


def test_guards():
    for dt in (torch.bfloat16, torch.float32):
        t = G.guard_fill(torch.empty(5, 7, dtype=dt))
        assert t.isnan().all() and G.guard_intact(t, torch.zeros(5, 7, dtype=torch.bool)) == 0
        t[2, 3] = float("nan")                                  # another NaN is not the guard
        assert G.guard_intact(t, torch.zeros(5, 7, dtype=torch.bool)) == 1
        w = torch.zeros(5, 7, dtype=torch.bool)
        w[2, 3] = True
        assert G.guard_intact(t, w) == 0


def test_inputs_are_poisoned_outside_what_the_contract_reads():
    c = G.CASE_BY_ID["n130_ldc131_f32"]
    b = G.build(c, 300, "cpu")
    assert b.A[:300, :c["K"]].isfinite().all() and b.A[:300, c["K"]:].isnan().all() and b.A[300:].isnan().all()
    assert b.B[:130, :c["K"]].isfinite().all() and b.B[130:].isnan().all()
    assert b.kw["bias"][:130].isfinite().all() and b.kw["bias"][130:134].isnan().all()
    assert b.kw["rowadd"].shape[0] == 7 and b.kw["rowadd"][:, 130:].isnan().all()
    cr = G.map_rows(c["cmap"], 300)
    keep = torch.zeros(b.kw["resid"].shape[0], dtype=torch.bool)
    keep[cr[cr >= 0]] = True
    assert b.kw["resid"][keep][:, :130].isfinite().all() and b.kw["resid"][~keep].isnan().all()
    assert b.full["C"].isnan().all() and b.full["C"].shape[0] == G.FRONT + b.lay.c_rows + G.BACK
    g = G.build(G.CASE_BY_ID["amap_gather"], 300, "cpu")
    ar = G.map_rows((75, 0, 96, 5), 300)
    used = torch.zeros(g.A.shape[0], dtype=torch.bool)
    used[ar] = True
    assert g.A[used][:, :192].isfinite().all() and g.A[~used].isnan().all() and int(used.sum()) == 300


# ------------------------------------------------------------------------------------------------ the dispatch table
PERSISTENT = ("w4", "p8", "p8@224", "p8@192", "p8@160")
FAMILIES = ("nt128", "big", "big2") + PERSISTENT
# what a family cannot take (gemm_plan.cpp w4_supported / p8_supported, short_tile): such a case runs on the fallback
_NO_PERSISTENT = {"amap_gather", "alpha", "pad4", "n_mod8"}
_SHORT_ACTS = {"act_none", "act_gelu_tanh"}


def _supports(fam, feats, c):
    if fam in PERSISTENT:
        if feats & _NO_PERSISTENT:
            return False
        if fam != "w4" and c["K"] < 128:
            return False
        if c["resid16"] and c["out"] != G.OUT_BF16:
            return False
        if "@" in fam and not ({f for f in feats if f.startswith("act_")} <= _SHORT_ACTS):
            return False
    return True


def test_plan_table_is_pinned_and_covers_every_family():
    from projectiontrainer_amd import _lib as L
    pinned = G.load_plan_table()
    now = G.plan_table(L, L.lib())
    assert now == pinned, sorted(k for k in now if now[k] != pinned.get(k))
    all_feats = set().union(*(G.features(c) for c in G.CASES))
    tile = {"nt128": (128, 128), "big": (256, 256), "big2": (256, 256), "w4": (256, 256), "p8": (256, 256),
            "p8@224": (224, 256), "p8@192": (192, 256), "p8@160": (160, 256)}
    ran = {f: {} for f in FAMILIES}          # family -> feature -> [ragged M seen, ragged N seen]
    for c in G.CASES:
        feats = G.features(c)
        for M in G.MS:
            for mode in G.MODES:
                fam = pinned[c["id"]][str(M)][str(mode)]
                assert fam in FAMILIES, (c["id"], M, mode, fam)
                assert _supports(fam, feats, c), (c["id"], M, mode, fam)
                th, tw = tile[fam]
                for f in feats:
                    seen = ran[fam].setdefault(f, [False, False])
                    seen[0] |= M % th != 0 and M > th
                    seen[1] |= c["N"] % tw != 0
    # (both M are ragged for every tile height, so the first flag is true by construction; the second is not: the
    # N % 128 == 0 cases are whole column tiles of the 128-wide family, N 256 of every family)
    missing = []
    for fam in FAMILIES:
        for f in sorted(all_feats - {"lean"}):      # ("lean" means whole column ranges: never ragged; held below)
            if not any(f in G.features(c) and _supports(fam, G.features(c), c) for c in G.CASES):
                assert fam in PERSISTENT, (fam, f)       # no case carries f in a form this family takes
                continue
            if ran[fam].get(f) != [True, True]:
                missing.append((fam, f, ran[fam].get(f)))
    assert not missing, missing
    # the lean epilogues' shapes (whole 128-column wave ranges) reach both persistent kernels, plain and GEGLU backward
    for fam in ("w4", "p8"):
        acts = {c["act"] for c in G.CASES if "lean" in G.features(c)
                and fam in pinned[c["id"]]["300"].values() and fam in pinned[c["id"]]["556"].values()}
        assert acts == {G.ACT_NONE, G.ACT_GELU_TANH, G.ACT_GEGLU_BWD}, (fam, acts)
    # the forced modes land where they say, and the second-round case on every persistent family
    r2 = pinned[G.ROUND2["id"]][str(G.ROUND2["M"])]
    assert [r2[str(m)] for m in G.ROUND2_MODES] == ["w4", "p8", "p8@224", "p8@192", "p8@160"]
    for fam, (th, tw) in tile.items():
        if fam in PERSISTENT:
            M, N = G.ROUND2["M"], G.ROUND2["N"]
            assert -(-M // th) * -(-N // tw) > 304           # more tiles than any MI355X partition has compute units
