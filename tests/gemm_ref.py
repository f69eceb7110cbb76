"""The contract of ptk_gemm_desc (include/ptk.h) restated in fp64, and the pieces the GEMM contract tests share
(tests/test_gemm_ref_cpu.py, tests/test_gemm_contract_gpu.py): the row map, operands whose products and sums are exact
in fp32 in any order, guard patterns for everything a launch must not touch, the case list and its dispatch table.
No project code is called by the reference: every function is written from the header and from the rounding points
of the epilogues (csrc/gemm_epi.h), with torch in fp64.

Order of operations for output row r, column c:
  1. v = alpha * sum_k A[amap(r)][k] B[c][k]          2. + bias[c]          3. bf16(v) if bf16_linear
  4. + rowadd[r % period][c]
  5. GELU-tanh / GELU-erf / GEGLU: the pre-activation is rounded to bf16 (and stored to aux at the UNMAPPED row r)
  6. the activation                                   7. stop if cmap(r) < 0; + resid / resid16 at the MAPPED row
  8. the output rounding (bf16, f32, f32 holding a bf16 value), stored at the mapped row.
Every rounding is one rounding of the fp64 value to bf16 (bfr: nearest, ties to even, on the fp64 bit pattern).

Exactness.  A holds integers in [-2, 2], B integers in [-4, 4] times 2^-6, K <= 320: every product and every partial
sum is a multiple of 2^-6 below 2^6, so fp32 accumulation is exact in any order; bias, rowadd and resid are multiples
of 2^-6 too, alpha is a power of two.  ACT_NONE outputs, the stored pre-activations and ACT_GEGLU_BWD (a product of
two bf16 values is exact in fp32: one rounding) are therefore compared bit for bit.  The transcendental epilogues
(GELU-tanh, GELU-erf, the GEGLU forward's a, b, h, GELU-erf backward) are compared with bf16(fp64 function of the exact
pre-activation) under two conditions: every element within REL_TOL |ref| + floor (one bf16 ulp; the floor covers the
far negative tail where 1 + erf(x) cancels in fp32), and the share of elements not bit-equal to the reference at most
NEQ_CAP."""
import json
import os
from types import SimpleNamespace

import torch

ACT_NONE, ACT_GELU_TANH, ACT_GELU_ERF, ACT_GEGLU, ACT_GELU_ERF_BWD, ACT_GEGLU_BWD = range(6)
OUT_BF16, OUT_F32, OUT_F32_BF16ROUND = range(3)
ACT_NAMES = ("none", "gelu_tanh", "gelu_erf", "geglu", "gelu_erf_bwd", "geglu_bwd")
EXACT_ACTS = (ACT_NONE, ACT_GEGLU_BWD)

REL_TOL = 2.0 ** -8
ABS_FLOOR = 2.0 ** -20
# Share of elements of a transcendental epilogue's output that may differ from bf16(fp64 function).  A condition, not a
# measurement: the fp32 restatement of the same formulas differs in at most 4.1e-5 of the samples at pre-activation
# std <= 1 (test_gemm_ref_cpu.py holds it to 1e-4), a missing or misplaced bf16 rounding moves tens of percent.
# Largest share seen on an MI355X over every case, M and force mode, on every family alike: MEASURED_NEQ (one element
# of 111 200 in gelu_erf_aux_grp at M 556, inside the absolute floor; every other transcendental output bit-equal).
NEQ_CAP = 2e-3
MEASURED_NEQ = {"gelu_tanh.C": 0.0, "gelu_erf.C": 9.0e-6, "geglu.aux": 0.0, "geglu.aux2": 0.0, "geglu.C": 0.0,
                "gelu_erf_bwd.C": 0.0}

GUARD_BF16 = 0x7FC5          # a quiet NaN with a payload no kernel produces
GUARD_F32 = 0x7FC5A5A5
FRONT, BACK = 16, 64         # spare rows in front of / behind every output buffer

MODES = (0, 1, 2, 4, 8, 32, 512, 1024, 4096)
MS = (300, 556)              # ragged for tile heights 128, 160, 192, 224 and 256; more than one row tile of each
PLAN_TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "gemm_contract_plan.json")
PLAN_NCU = 256


# ------------------------------------------------------------------------------------------------ small helpers
def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def guard_fill(t):
    """Every element of t becomes the guard NaN of its type."""
    bits(t).fill_(GUARD_BF16 if t.dtype == torch.bfloat16 else GUARD_F32)
    return t


def guard_intact(t, written):
    """Number of elements outside `written` (bool, t's shape) that no longer hold the guard pattern."""
    g = GUARD_BF16 if t.dtype == torch.bfloat16 else GUARD_F32
    return int(((bits(t) != g) & ~written).sum())


def nan_buffer(rows, ld, dtype, device):
    return torch.full((rows, ld), float("nan"), dtype=dtype, device=device)


def bfr(x):
    """bf16 rounding (nearest, ties to even) of an fp64 tensor, back in fp64: the fp64 value itself is rounded to 8
    significant bits and then passes through fp32 and .to(torch.bfloat16) unchanged.  Taking an fp64 value to fp32
    first would round twice: gelu'(g) u = 1.003906289545 (a real element of the geglu_grp case) lies 3.9e-8 above
    the tie 1 + 2^-8, fp32 rounds it onto the tie and bf16 then ties to even, 1.0, where bf16 of the fp64 value is
    1.0078125.  For the dyadic sums, which fp32 holds exactly, the two routes are the same."""
    # on the fp64 bit pattern (integer arithmetic: the same on every device, where frexp / ldexp need not be exact):
    # 45 of the 52 fraction bits go, half of the kept unit minus one plus the kept unit's parity is added first (a
    # carry out of the fraction raises the exponent, as it should)
    b = x.double().contiguous().view(torch.int64)
    b = (b + ((1 << 44) - 1) + ((b >> 45) & 1)) & -(1 << 45)
    r = b.view(torch.float64)
    out = r.to(torch.float32).to(torch.bfloat16).double()
    assert bool(((out == r) | ~torch.isfinite(r)).all()), "bfr: a value outside bf16's normal range"
    return out


def map_row(g, skip, gs, off, r):
    """ptk_rowmap: r -> (r / g) * gs + r % g + off, -1 (dropped) where r % g < skip; g == 0: r + off, dropped
    where that is negative."""
    if g == 0:
        return r + off if r + off >= 0 else -1
    q, s = divmod(r, g)
    if s < skip:
        return -1
    return q * gs + s + off


def map_rows(m, M, device=None):
    """map_row over r = 0 .. M-1 as an int64 tensor (vectorised; test_gemm_ref_cpu.py holds it to the loop)."""
    g, skip, gs, off = m
    r = torch.arange(M, dtype=torch.int64, device=device)
    if g == 0:
        c = r + off
        return torch.where(c >= 0, c, torch.full_like(c, -1))
    q, s = r // g, r % g
    return torch.where(s < skip, torch.full_like(r, -1), q * gs + s + off)


def dyadic(shape, lo, hi, shift, seed, dtype=torch.bfloat16):
    """Integers in [lo, hi] times 2^-shift (CPU generator: the same values on every machine)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(lo, hi + 1, tuple(shape), generator=g, dtype=torch.int32).double() * 2.0 ** -shift).to(dtype)


# ------------------------------------------------------------------------------------------------ activations, fp64
K0, K1 = 0.7978845608028654, 0.044715


def gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(K0 * (x + K1 * x ** 3)))


def gelu_tanh_grad(x):
    t = torch.tanh(K0 * (x + K1 * x ** 3))
    return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * K0 * (1.0 + 3.0 * K1 * x * x)


def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))


def gelu_erf_grad(x):
    return 0.5 * (1.0 + torch.erf(x * 0.7071067811865476)) + x * 0.3989422804014327 * torch.exp(-0.5 * x * x)


# The same four forms in fp32, as a kernel would write them (exp2 / reciprocal for the tanh form, erf / exp for the erf
# form): only to show on the CPU that fp32 evaluation alone stays far inside NEQ_CAP.
def f32_gelu_tanh(x):
    e = torch.exp2(x * (x * x * (K0 * K1 * -2.8853900817779268) + K0 * -2.8853900817779268))
    return x * (1.0 / (1.0 + e))


def f32_geglu_b(g, u):
    x2 = g * g
    e = torch.exp2(g * (x2 * (K0 * K1 * -2.8853900817779268) + K0 * -2.8853900817779268))
    s = 1.0 / (1.0 + e)
    f = g * s
    return ((f - f * s) * (x2 * (6.0 * K0 * K1) + 2.0 * K0) + s) * u


def f32_gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))


def f32_gelu_erf_bwd(dh, x):
    return dh * (0.5 * (1.0 + torch.erf(x * 0.7071067811865476)) + x * 0.3989422804014327 * torch.exp(-0.5 * x * x))


# ------------------------------------------------------------------------------------------------ the reference
def _ld(t):
    return t.stride(0)


def _gather(t, base, rows, ld, ncol):
    """t (a contiguous buffer whose element 0 is the descriptor's pointer)[base + rows * ld + 0..ncol) in fp64."""
    idx = base + rows[:, None] * ld + torch.arange(ncol, device=t.device)[None, :]
    return t.reshape(-1)[idx].double(), idx


def ref(A, B, *, C, M, N, K, act=ACT_NONE, alpha=1.0, bias=None, rowadd=None, resid=None, aux=None, aux2=None,
        aux_in=None, aux_in2=None, batch=1, batch_inner=1, strides=(0, 0, 0, 0, 0, 0), amap=(0, 0, 0, 0),
        cmap=(0, 0, 0, 0), out_mode=None, resid16=None, bf16_linear=False):
    """Expected contents of C, aux and aux2 after ptk_gemm of this descriptor, as full buffers: every tensor is a
    contiguous 2-D buffer [rows, ld] whose first element is what the descriptor points at (batches and row maps
    address past its rows through the strides), holding its contents before the launch.  Returns a namespace with,
    for each name in outs ("C", "aux", "aux2"), exp[name] (the buffer after the launch) and written[name] (bool: the
    elements the launch stores), and scale (max |dh| of a GELU-erf backward, for its absolute floor)."""
    dev = A.device
    if out_mode is None:
        out_mode = OUT_BF16 if C.dtype == torch.bfloat16 else OUT_F32
    n_out = N // 2 if act == ACT_GEGLU else 2 * N if act == ACT_GEGLU_BWD else N
    exp = {"C": C.clone()}
    written = {"C": torch.zeros(C.shape, dtype=torch.bool, device=dev)}
    for name, t in (("aux", aux), ("aux2", aux2)):
        if t is not None and act in (ACT_GELU_TANH, ACT_GELU_ERF, ACT_GEGLU):
            exp[name] = t.clone()
            written[name] = torch.zeros(t.shape, dtype=torch.bool, device=dev)
    r = torch.arange(M, dtype=torch.int64, device=dev)
    ar, cr = map_rows(amap, M, dev), map_rows(cmap, M, dev)
    assert int(ar.min()) >= 0, "amap must map every row"
    keep = cr >= 0
    scale = 0.0
    sA0, sA1, sB0, sB1, sC0, sC1 = strides
    for z in range(batch):
        z0, z1 = divmod(z, batch_inner)
        a, _ = _gather(A, z0 * sA0 + z1 * sA1, ar, _ld(A), K)
        b, _ = _gather(B, z0 * sB0 + z1 * sB1, torch.arange(N, device=dev), _ld(B), K)
        v = alpha * (a @ b.T)
        if bias is not None:
            v = v + bias.reshape(-1)[:N].double()[None, :]
        if bf16_linear:
            v = bfr(v)
        if rowadd is not None:
            v = v + _gather(rowadd, 0, r % rowadd.shape[0], _ld(rowadd), N)[0]
        side = {}
        if act in (ACT_GELU_TANH, ACT_GELU_ERF):
            v = bfr(v)
            side["aux"] = v
            v = gelu_tanh(v) if act == ACT_GELU_TANH else gelu_erf(v)
        elif act == ACT_GELU_ERF_BWD:
            v = bfr(v)
            scale = max(scale, float(v.abs().max()))
            v = v * gelu_erf_grad(_gather(aux_in, 0, r, _ld(aux_in), N)[0])
        elif act == ACT_GEGLU:     # columns [32q, 32q + 16) gate, [32q + 16, 32q + 32) up of h columns [16q, 16q + 16)
            v4 = bfr(v).reshape(M, N // 32, 2, 16)
            g, u = v4[:, :, 0, :].reshape(M, N // 2), v4[:, :, 1, :].reshape(M, N // 2)
            fa = bfr(gelu_tanh(g))
            side["aux"], side["aux2"] = fa, bfr(gelu_tanh_grad(g) * u)
            v = bfr(fa * u)
        elif act == ACT_GEGLU_BWD:  # dg = bf16(dh) * b, du = bf16(dh) * a into the interleaved [M, 2N] layout
            dh = bfr(v)
            fa, fb = _gather(aux_in, 0, r, _ld(aux_in), N)[0], _gather(aux_in2, 0, r, _ld(aux_in), N)[0]
            v = torch.stack([(dh * fb).reshape(M, N // 16, 16), (dh * fa).reshape(M, N // 16, 16)], 2).reshape(M, 2 * N)
        for name, val in side.items():
            if name in exp:            # at the unmapped row (GELU-tanh's needs an identity cmap: the same row)
                t = (aux, aux2)[name == "aux2"]
                idx = r[:, None] * _ld(t) + torch.arange(val.shape[1], device=dev)[None, :]
                exp[name].reshape(-1)[idx] = val.to(torch.float32).to(t.dtype)
                written[name].reshape(-1)[idx] = True
        v, crk = v[keep], cr[keep]
        if resid is not None:
            v = v + _gather(resid, 0, crk, _ld(resid), n_out)[0]
        if resid16 is not None:
            v = v + _gather(resid16, 0, crk, _ld(resid16), n_out)[0]
        if out_mode != OUT_F32:
            v = bfr(v)
        idx = (z0 * sC0 + z1 * sC1) + crk[:, None] * _ld(C) + torch.arange(n_out, device=dev)[None, :]
        exp["C"].reshape(-1)[idx] = v.to(torch.float32).to(C.dtype)
        written["C"].reshape(-1)[idx] = True
    return SimpleNamespace(exp=exp, written=written, scale=scale, exact=act in EXACT_ACTS, act=act)


def compare(got, want, written, exact, floor=ABS_FLOOR):
    """(elements written, not bit-equal among them, outside REL_TOL |ref| + floor among them, the largest error as
    a multiple of that bound).  exact: any bit difference counts as outside."""
    neq = (bits(got) != bits(want)) & written
    n, nneq = int(written.sum()), int(neq.sum())
    if nneq == 0:
        return n, 0, 0, 0.0
    g, w = got.double(), want.double()
    ratio = torch.where(neq, (g - w).abs() / (REL_TOL * w.abs() + floor), torch.zeros_like(w))
    ratio = torch.where(ratio.isnan(), torch.full_like(ratio, float("inf")), ratio)      # (a NaN is outside)
    return n, nneq, nneq if exact else int((ratio > 1.0).sum()), float(ratio.max())


# ------------------------------------------------------------------------------------------------ the cases
# A case is plain data (no tensors), so the CPU test can plan it and the GPU test can build it.  Fields (defaults in
# case()): N, K, act, out, alpha, bias, rowadd (period, 0: none), resid / resid16 (None, "alias": C itself, "own": its own
# buffer), bf16_linear, aux (side outputs where the activation has them), amap, cmap, pad (added to every leading
# dimension; 4: lda / ldb, which must stay 16-byte rows, get 8), pad_<name> (one leading dimension), ldc (absolute).
CASES = []
_K_ROT = (192, 64, 320, 128)


def case(cid, **kw):
    c = dict(id=cid, N=320, K=_K_ROT[len(CASES) % 4], act=ACT_NONE, out=OUT_BF16, alpha=1.0, bias=False, rowadd=0,
             resid=None, resid16=None, bf16_linear=False, aux=False, amap=(0, 0, 0, 0), cmap=(0, 0, 0, 0), pad=0)
    c.update(kw)
    assert c["id"] not in {x["id"] for x in CASES}
    CASES.append(c)


LOSSMAP = (75, 0, 96, 21)    # (text rows, 0, padded sequence, first loss row): the last Gemma3 layer's loss rows
OUTS = ((OUT_BF16, "bf16"), (OUT_F32, "f32"), (OUT_F32_BF16ROUND, "f32r"))

# row maps on A
case("amap_off24", amap=(0, 0, 0, 24), K=128)
case("amap_off16_n200", amap=(0, 0, 0, 16), N=200, K=64)
case("amap_gather", amap=(75, 0, 96, 5), K=192)
case("amap_gather_n200", amap=(75, 0, 96, 5), N=200, K=320)
case("lossmap_geglu", act=ACT_GEGLU, N=352, K=128, amap=LOSSMAP, aux=True)          # models.cpp: the last layer's MLP
case("lossmap_geglu_n320", act=ACT_GEGLU, N=320, K=192, amap=LOSSMAP, aux=True)
# row maps on C
case("cmap_off", cmap=(0, 0, 0, 24))
case("cmap_off_n200", cmap=(0, 0, 0, 24), N=200)
case("cmap_group", cmap=(60, 0, 80, 3))
case("cmap_group_n200", cmap=(60, 0, 80, 3), N=200)
case("cmap_skip", cmap=(60, 1, 80, -1))
case("cmap_skip_n200", cmap=(60, 1, 80, -1), N=200)
case("cmap_neg", cmap=(0, 0, 0, -7))
case("cmap_neg_n200", cmap=(0, 0, 0, -7), N=200)
case("cmap_identity_group", cmap=(128, 0, 128, 0))
case("cmap_identity_group_n200", cmap=(128, 0, 128, 0), N=200)
case("lossmap_scatter", cmap=LOSSMAP, K=320)                                        # the compact result scattered back
case("lossmap_scatter_n200", cmap=LOSSMAP, N=200, K=128)
# additive inputs, each with every output mode it is allowed under
for o, on in OUTS:
    case(f"bias_{on}", bias=True, out=o)
    case(f"bias_n200_{on}", bias=True, out=o, N=200)
    case(f"rowadd7_{on}", rowadd=7, pad_rowadd=4, out=o)
    case(f"rowadd37_n200_{on}", rowadd=37, pad_rowadd=4, out=o, N=200, cmap=(60, 0, 80, 3))
    case(f"resid_own_{on}", resid="own", pad_resid=4, out=o, cmap=(60, 0, 80, 3))
    case(f"resid_own_n200_{on}", resid="own", pad_resid=4, out=o, N=200)
    case(f"alpha_{on}", alpha=0.5, out=o)
    case(f"alpha_bias_n200_{on}", alpha=0.5, bias=True, out=o, N=200)
    case(f"chain_{on}", bias=True, rowadd=37, resid="own", bf16_linear=True, out=o, N=200, cmap=(60, 1, 80, -1))
for o, on in OUTS[1:]:                                                              # (resid is fp32: an fp32 C)
    case(f"resid_alias_{on}", resid="alias", out=o)
    case(f"resid_alias_n200_{on}", resid="alias", out=o, N=200, cmap=(60, 0, 80, 3))
for lin in (False, True):
    case(f"resid16_alias_lin{int(lin)}", resid16="alias", bf16_linear=lin, bias=True)
    case(f"resid16_alias_n200_lin{int(lin)}", resid16="alias", bf16_linear=lin, N=200, cmap=(0, 0, 0, 24))
    case(f"resid16_own_lin{int(lin)}", resid16="own", bf16_linear=lin, bias=lin)
    case(f"resid16_own_n200_lin{int(lin)}", resid16="own", bf16_linear=lin, bias=True, rowadd=7, N=200,
         cmap=(60, 0, 80, 3))
# leading dimensions
case("pad8_plain", pad=8)
case("pad8_lean_resid16", pad=8, bias=True, resid16="own", bf16_linear=True, cmap=(0, 0, 0, 24))
for o, on in OUTS:
    case(f"pad8_chain_n200_{on}", pad=8, bias=True, rowadd=7, resid="own", out=o, N=200, cmap=(60, 0, 80, 3))
    case(f"pad4_chain_{on}", pad=4, bias=True, rowadd=7, resid="own", out=o, cmap=(60, 0, 80, 3))
case("pad4_resid16_n200", pad=4, bias=True, resid16="own", bf16_linear=True, N=200)
# N = 130: the scalar epilogue (ldc 131: no vector access is possible) and the 4-column one with a scalar tail (132)
for o, on in OUTS:
    case(f"n130_ldc131_{on}", N=130, ldc=131, pad_resid=1, pad_rowadd=1, bias=True, rowadd=7, resid="own",
         bf16_linear=True, out=o, cmap=(60, 1, 80, -1))
    case(f"n130_ldc132_{on}", N=130, ldc=132, pad_resid=2, pad_rowadd=2, bias=True, rowadd=37, resid="own", out=o,
         cmap=(60, 0, 80, 3))
case("n130_ldc131_resid16", N=130, ldc=131, pad_resid16=1, bias=True, resid16="own", bf16_linear=True)
case("n130_ldc136_resid16", N=130, ldc=136, pad_resid16=6, bias=True, resid16="alias", bf16_linear=True)
# activations x {identity, offset, group} C row maps, with the side outputs / inputs where they exist
_CM = (("id", (0, 0, 0, 0)), ("off", (0, 0, 0, 24)), ("grp", (60, 0, 80, 3)))
for cn, cm in _CM:
    n = 320 if cn == "id" else 200
    case(f"gelu_tanh_{cn}", act=ACT_GELU_TANH, cmap=cm, N=n, bias=True)
    case(f"gelu_erf_{cn}", act=ACT_GELU_ERF, cmap=cm, N=n, bias=True)
    case(f"gelu_erf_aux_{cn}", act=ACT_GELU_ERF, cmap=cm, N=n, bias=True, aux=True, pad_aux=8)
    case(f"gelu_erf_bwd_{cn}", act=ACT_GELU_ERF_BWD, cmap=cm, N=n, pad_aux_in=8)
    case(f"geglu_{cn}", act=ACT_GEGLU, cmap=cm, N=320 if cn == "id" else 352, aux=True)
    case(f"geglu_noaux_{cn}", act=ACT_GEGLU, cmap=cm, N=352 if cn == "id" else 320)
    case(f"geglu_bwd_{cn}", act=ACT_GEGLU_BWD, cmap=cm, N=160 if cn == "id" else 208, pad_aux_in=8)
case("gelu_tanh_aux", act=ACT_GELU_TANH, bias=True, aux=True)                        # (ld_aux == ldc, identity cmap)
case("gelu_tanh_aux_n200", act=ACT_GELU_TANH, bias=True, aux=True, N=200, pad=8)
case("gelu_tanh_rowadd", act=ACT_GELU_TANH, rowadd=7, N=200)
case("gelu_tanh_lean_off", act=ACT_GELU_TANH, bias=True, cmap=(0, 0, 0, 24), N=320)
case("geglu_pad4", act=ACT_GEGLU, N=352, aux=True, pad=4, cmap=(60, 0, 80, 3))
case("geglu_bwd_pad4", act=ACT_GEGLU_BWD, N=208, pad=4, cmap=(60, 0, 80, 3))
case("geglu_bwd_n160_grp", act=ACT_GEGLU_BWD, N=160, pad=8, cmap=(60, 1, 80, -1))
# each non-interleaved activation under a ragged N
case("gelu_tanh_n130", act=ACT_GELU_TANH, N=130, ldc=131, bias=True, aux=True, pad_aux=1)
case("gelu_erf_n130", act=ACT_GELU_ERF, N=130, ldc=132, bias=True, aux=True, pad_aux=3, cmap=(60, 0, 80, 3))
case("gelu_erf_bwd_n130", act=ACT_GELU_ERF_BWD, N=130, ldc=131, pad_aux_in=1, cmap=(0, 0, 0, 24))
# (new cases go below: a case's operands are seeded by its position in the list)
# resid16 into an fp32 C, with and without bf16_linear: the 8-, 4-column and scalar epilogues of the 128x128 / 256x256
# kernels (the persistent kernels take resid16 with a bf16 C only, so these run on the fallback under every mode)
for o, on in OUTS[1:]:
    for lin in (False, True):
        case(f"resid16_own_{on}_lin{int(lin)}", resid16="own", bf16_linear=lin, bias=True, out=o, cmap=(60, 0, 80, 3))
        case(f"resid16_own_n200_{on}_lin{int(lin)}", resid16="own", pad_resid16=4, bf16_linear=lin, bias=lin, out=o,
             N=200, cmap=(0, 0, 0, 24))
    case(f"n130_ldc132_resid16_{on}", N=130, ldc=132, pad_resid16=6, bias=True, resid16="own", bf16_linear=True, out=o)
    case(f"n130_ldc131_resid16_{on}", N=130, ldc=131, pad_resid16=1, resid16="own", out=o, cmap=(60, 1, 80, -1))
# N % 128 == 0: whole 128-column wave ranges, where the persistent kernels take their lean epilogues (gemm_plan.cpp
# lean_epilogue_ok, lean_glu_ok; launch_gemm_w4) -- plain / GELU-tanh with a bias, the bf16-linear rounding and a bf16
# residual under an offset C row map, and the lean GEGLU backward.  Rows past M and the rows behind C are dropped by
# the store resource's range there, not by a per-row test: the guards behind C are what checks it
case("lean_n384_plain", N=384, K=192)
case("lean_n384_resid16_off", N=384, K=128, bias=True, resid16="own", bf16_linear=True, cmap=(0, 0, 0, 24))
case("lean_n256_resid16_alias", N=256, K=320, bias=True, resid16="alias", cmap=(128, 0, 128, 0))
case("lean_n384_pad8_off", N=384, K=192, pad=8, bias=True, resid16="own", cmap=(0, 0, 0, 16))
case("lean_gelu_tanh_n384_off", act=ACT_GELU_TANH, N=384, K=128, bias=True, bf16_linear=True, cmap=(0, 0, 0, 24))
case("lean_gelu_tanh_n256", act=ACT_GELU_TANH, N=256, K=192, bias=True, cmap=(128, 0, 128, 0))
case("lean_geglu_bwd_n128", act=ACT_GEGLU_BWD, N=128, K=128)
case("lean_geglu_bwd_n256_off", act=ACT_GEGLU_BWD, N=256, K=192, cmap=(0, 0, 0, 24))
case("lean_geglu_bwd_n256_pad8", act=ACT_GEGLU_BWD, N=256, K=320, pad=8, cmap=(128, 0, 128, 0))

CASE_BY_ID = {c["id"]: c for c in CASES}

# the persistent families' second tile round: more tiles than the device has compute units, a group cmap and an fp32
# resid (a workgroup's second tile derives its row state again)
ROUND2 = dict(id="round2", M=4396, N=4160, K=128, act=ACT_NONE, out=OUT_F32, alpha=1.0, bias=True, rowadd=0,
              resid="own", resid16=None, bf16_linear=False, aux=False, amap=(0, 0, 0, 0), cmap=(1099, 0, 1100, 2), pad=0)
ROUND2_MODES = (8, 32, 512, 1024, 4096)

# features a case exercises (the coverage table of test_gemm_ref_cpu.py)
def features(c):
    f = {"act_" + ACT_NAMES[c["act"]], ("out_bf16", "out_f32", "out_f32r")[c["out"]]}
    g, skip, gs, off = c["amap"]
    if g:
        f.add("amap_gather")
    elif off:
        f.add("amap_off")
    g, skip, gs, off = c["cmap"]
    if g == 0 and off > 0:
        f.add("cmap_off")
    if g == 0 and off < 0:
        f.add("cmap_neg")
    if g and skip:
        f.add("cmap_skip")
    if g and not skip:
        f.add("cmap_group")
    for k in ("bias", "rowadd", "bf16_linear"):
        if c[k]:
            f.add(k)
    if c["alpha"] != 1.0:
        f.add("alpha")
    for k in ("resid", "resid16"):
        if c[k]:
            f.add(f"{k}_{c[k]}")
    if c["aux"]:
        f.add("aux")
    if c["act"] in (ACT_GELU_ERF_BWD, ACT_GEGLU_BWD):
        f.add("aux_in")
    if c["pad"]:
        f.add(f"pad{c['pad']}")
    if c["N"] % 8:
        f.add("n_mod8")
    # what gemm_plan.cpp's lean_epilogue_ok / lean_glu_ok and launch_gemm_w4 ask of a descriptor, on both persistent
    # kernels: the shapes whose stores and residual loads go through range-checked buffer resources
    g, skip, gs, off = c["cmap"]
    affine = off >= 0 and (g == 0 or (skip == 0 and g == gs))
    plain = c["act"] in (ACT_NONE, ACT_GELU_TANH) and not (c["rowadd"] or c["resid"] or c["aux"])
    glu = c["act"] == ACT_GEGLU_BWD
    if (plain or glu) and affine and c["out"] == OUT_BF16 and c["N"] % 128 == 0 and c["alpha"] == 1.0 and \
            c["pad"] in (0, 8) and not c["amap"][0]:
        f.add("lean")
    return f


# ------------------------------------------------------------------------------------------------ layout and build
def layout(c, M):
    """The descriptor's scalar fields for case c at M rows: sizes, leading dimensions, buffer row counts."""
    N, K, act = c["N"], c["K"], c["act"]
    pad = c["pad"]
    n_out = N // 2 if act == ACT_GEGLU else 2 * N if act == ACT_GEGLU_BWD else N
    n_aux = N // 2 if act == ACT_GEGLU else N
    p = lambda name, width: width + c.get("pad_" + name, pad)
    lay = SimpleNamespace(M=M, N=N, K=K, n_out=n_out, n_aux=n_aux)
    lay.lda = lay.ldb = K + (8 if pad else 0)
    lay.ldc = c.get("ldc", n_out + pad)
    lay.ld_resid = lay.ldc if c["resid"] == "alias" else p("resid", n_out)
    lay.ld_resid16 = lay.ldc if c["resid16"] == "alias" else p("resid16", n_out)
    lay.ld_rowadd = p("rowadd", N)
    lay.ld_aux = lay.ldc if (act == ACT_GELU_TANH and c["aux"]) else p("aux", n_aux)
    lay.ld_aux_in = p("aux_in", N)
    lay.a_rows = max(map_row(*c["amap"], r) for r in range(M)) + 1
    lay.c_rows = max(max(map_row(*c["cmap"], r) for r in range(M)) + 1, 1)
    return lay


def desc(L, c, M, ptrs=None):
    """ptk_gemm_desc of case c at M rows; ptrs: {field: address} (default: distinct 16-byte aligned fake addresses,
    for the host-side planner, which reads only their alignment and presence)."""
    lay, act = layout(c, M), c["act"]
    fake = iter(range(0x10000000, 0x70000000, 0x04000000))
    P = lambda name, present=True: (ptrs[name] if ptrs else next(fake)) if present else None
    d = L.GemmDesc()
    d.A, d.B, d.C = P("A"), P("B"), P("C")
    d.M, d.N, d.K = M, c["N"], c["K"]
    d.lda, d.ldb, d.ldc = lay.lda, lay.ldb, lay.ldc
    d.batch, d.batch_inner = 1, 1
    d.alpha, d.act, d.out = c["alpha"], act, c["out"]
    d.bias = P("bias", c["bias"])
    if c["rowadd"]:
        d.rowadd, d.rowadd_period, d.ld_rowadd = P("rowadd"), c["rowadd"], lay.ld_rowadd
    if c["resid"]:
        d.resid, d.ld_resid = (d.C if c["resid"] == "alias" else P("resid")), lay.ld_resid
    if c["resid16"]:
        d.resid16, d.ld_resid16 = (d.C if c["resid16"] == "alias" else P("resid16")), lay.ld_resid16
    if c["aux"]:
        d.aux, d.ld_aux = P("aux"), lay.ld_aux
        if act == ACT_GEGLU:
            d.aux2 = P("aux2")
    if act in (ACT_GELU_ERF_BWD, ACT_GEGLU_BWD):
        d.aux_in, d.ld_aux_in = P("aux_in"), lay.ld_aux_in
        if act == ACT_GEGLU_BWD:
            d.aux_in2 = P("aux_in2")
    d.amap, d.cmap = L.RowMap(*c["amap"]), L.RowMap(*c["cmap"])
    d.bf16_linear = int(c["bf16_linear"])
    return d


def family(L, lib, d, mode, ncu=PLAN_NCU):
    """The family the planner gives descriptor d under force mode `mode`: the census name, "p8@224" etc. for the
    8-wave kernel's short tiles.  Sets and leaves the force mode."""
    import ctypes
    L.check(lib.ptk_gemm_force_small_tiles(mode), "force")
    path, tm = ctypes.c_int(-1), ctypes.c_int(-1)
    L.check(lib.ptk_gemm_plan(d, ncu, ctypes.byref(path), ctypes.byref(tm), None), "ptk_gemm_plan")
    name = L.GEMM_PATHS[path.value]
    return name if tm.value in (0, 256) or name != "p8" else f"p8@{tm.value}"


def plan_table(L, lib):
    """{case id: {M: {mode: family}}} under ncu 256, the pinned table's content."""
    t = {}
    try:
        for c in CASES:
            t[c["id"]] = {str(M): {str(m): family(L, lib, desc(L, c, M), m) for m in MODES} for M in MS}
        t[ROUND2["id"]] = {str(ROUND2["M"]): {str(m): family(L, lib, desc(L, ROUND2, ROUND2["M"]), m)
                                              for m in ROUND2_MODES}}
    finally:
        lib.ptk_gemm_force_small_tiles(0)
    return t


def write_plan_table():
    """Regenerate tests/data/gemm_contract_plan.json (python -c "from tests import gemm_ref as G;
    G.write_plan_table()") after a deliberate change of a dispatch rule or of the case list."""
    from projectiontrainer_amd import _lib as L
    with open(PLAN_TABLE, "w") as f:
        json.dump({"ncu": PLAN_NCU, "plan": plan_table(L, L.lib())}, f, indent=0, sort_keys=True)
        f.write("\n")


def load_plan_table():
    with open(PLAN_TABLE) as f:
        t = json.load(f)
    assert t["ncu"] == PLAN_NCU
    return t["plan"]


def _out_buffer(rows, ld, dtype, device):
    """(full guard-filled buffer [FRONT + rows + BACK, ld], the view the descriptor points at)."""
    full = guard_fill(torch.empty((FRONT + rows + BACK, ld), dtype=dtype, device=device))
    return full, full[FRONT:]


def _in_buffer(rows, ld, dtype, device, row_idx, ncol, values):
    """(full NaN buffer with FRONT / 8 spare rows, its pointed-at view) holding `values` at rows row_idx, columns
    0..ncol: every element the contract does not read is NaN."""
    full = nan_buffer(FRONT + rows + 8, ld, dtype, device)
    view = full[FRONT:]
    view[row_idx, :ncol] = values.to(device=device, dtype=dtype)
    return full, view


def build(c, M, device, seed=0):
    """Tensors of case c at M rows on `device`: a namespace with A, B, kw (the keyword arguments of kernels.gemm and
    of ref), full (name -> the whole buffer of every output, guards included), view (name -> the pointed-at view) and
    init (name -> a copy of an output's contents before the launch, to restore it between launches)."""
    lay, act, N, K = layout(c, M), c["act"], c["N"], c["K"]
    s = 1000 * (CASES.index(c) + 1 if c in CASES else 999) + (M % 97) * 7 + seed
    f32, b16 = torch.float32, torch.bfloat16
    rows = torch.arange(M)
    ar = map_rows(c["amap"], M)
    cr = map_rows(c["cmap"], M)
    crk = cr[cr >= 0]
    _, A = _in_buffer(lay.a_rows, lay.lda, b16, device, ar, K, dyadic((M, K), -2, 2, 0, s + 1))
    _, B = _in_buffer(N, lay.ldb, b16, device, torch.arange(N), K, dyadic((N, K), -4, 4, 6, s + 2))
    out_dt = b16 if c["out"] == OUT_BF16 else f32
    full, view = {}, {}
    full["C"], view["C"] = _out_buffer(lay.c_rows, lay.ldc, out_dt, device)
    kw = dict(C=view["C"], M=M, N=N, K=K, act=act, alpha=c["alpha"], amap=c["amap"], cmap=c["cmap"],
              out_mode=c["out"], bf16_linear=c["bf16_linear"])
    small = act != ACT_NONE          # (pre-activation std <= 1: the additive inputs stay small under an activation)
    if c["bias"]:
        kw["bias"] = _in_buffer(1, N + 4, f32, device, torch.zeros(1, dtype=torch.long), N,
                                dyadic((1, N), -16, 16, 6, s + 3, f32))[1].reshape(-1)
    if c["rowadd"]:
        kw["rowadd"] = _in_buffer(c["rowadd"], lay.ld_rowadd, f32, device, torch.arange(c["rowadd"]), N,
                                  dyadic((c["rowadd"], N), -16 if small else -64, 16 if small else 64, 6, s + 4, f32))[1][:c["rowadd"]]
    for name, dt, ld in (("resid", f32, lay.ld_resid), ("resid16", b16, lay.ld_resid16)):
        if not c[name]:
            continue
        vals = dyadic((len(crk), lay.n_out), -64, 64, 6, s + 5, dt)
        if c[name] == "alias":
            view["C"][crk.to(device), :lay.n_out] = vals.to(device)
            kw[name] = view["C"]
        else:
            kw[name] = _in_buffer(lay.c_rows, ld, dt, device, crk, lay.n_out, vals)[1]
    if c["aux"]:
        full["aux"], view["aux"] = _out_buffer(M, lay.ld_aux, b16, device)
        kw["aux"] = view["aux"]
        if act == ACT_GEGLU:
            full["aux2"], view["aux2"] = _out_buffer(M, lay.ld_aux, b16, device)
            kw["aux2"] = view["aux2"]
    if act in (ACT_GELU_ERF_BWD, ACT_GEGLU_BWD):
        kw["aux_in"] = _in_buffer(M, lay.ld_aux_in, b16, device, rows, N, dyadic((M, N), -96, 96, 6, s + 6))[1]
        if act == ACT_GEGLU_BWD:
            kw["aux_in2"] = _in_buffer(M, lay.ld_aux_in, b16, device, rows, N, dyadic((M, N), -96, 96, 6, s + 7))[1]
    init = {k: v.clone() for k, v in full.items()}
    alias = "alias" in (c["resid"], c["resid16"])
    return SimpleNamespace(A=A, B=B, kw=kw, full=full, view=view, init=init, lay=lay, alias=alias)


def restore(b):
    """Put every output buffer of build() back to its contents before the launch."""
    for k, v in b.full.items():
        v.copy_(b.init[k])


def measure(full, init, view, r, name, alias=False):
    """Figures of one output buffer after a launch against ref() r: (written, not bit-equal, outside the bound, the
    largest error as a multiple of the bound, elements outside the written set that changed, guard elements lost)."""
    wr = r.written[name]
    pre = name == "aux" and r.act in (ACT_GELU_TANH, ACT_GELU_ERF)       # a stored pre-activation: exact
    floor = ABS_FLOOR * (r.scale if r.act == ACT_GELU_ERF_BWD else 1.0)
    n, neq, bad, worst = compare(view, r.exp[name], wr, r.exact or pre, floor)
    # untouched: the front and back guard rows, the ld padding, dropped rows
    wfull = torch.zeros(full.shape, dtype=torch.bool, device=full.device)
    wfull[full.shape[0] - wr.shape[0]:] = wr
    stray = int(((bits(full) != bits(init)) & ~wfull).sum())
    lost = 0 if alias else guard_intact(full, wfull)   # (a C that is also the residual holds values, all overwritten)
    return n, neq, bad, worst, stray, lost


def check(b, r, label=""):
    """Compare the buffers of build() b after a launch with ref() r: bit equality (exact epilogues, and every stored
    pre-activation) or the two conditions, and the guards.  Every figure is printed.  Returns ({name: (written, not
    bit-equal)}, [what failed]): the caller asserts the list empty once all its launches are measured."""
    stats, failed = {}, []
    for name in r.exp:
        n, neq, bad, worst, stray, lost = measure(b.full[name], b.init[name], b.view[name], r, name,
                                                  name == "C" and b.alias)
        stats[name] = (n, neq)
        line = (f"{label} {name}: written {n} not-bit-equal {neq} outside-bound {bad} worst {worst:.3f}x "
                f"stray {stray} guard-lost {lost}")
        print(line)
        if not (n > 0 and bad == 0 and neq <= NEQ_CAP * n and stray == 0 and lost == 0):
            failed.append(line)
    return stats, failed
