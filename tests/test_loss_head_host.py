"""The test-facing entries of the loss head (include/ptk.h: ptk_gemm_row_stats, ptk_cross_entropy_stats,
ptk_count_valid, ptk_loss_reduce): exported and bound, and their argument validation, which runs before any device
call and so holds without a GPU.  Host memory stands in for the device buffers and must come back untouched.  Also
the fp64 helpers of tests/loss_util.py against torch's own fp64 cross entropy."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests import loss_util as U

NEW = ["ptk_gemm_row_stats", "ptk_cross_entropy_stats", "ptk_count_valid", "ptk_loss_reduce"]


@pytest.fixture(scope="module")
def env():
    from projectiontrainer_amd import _lib as L
    buf = (ctypes.c_char * 4096)(*([0x5A] * 4096))
    return L, L.lib(), buf, (ctypes.addressof(buf) + 63) & ~63        # (the pointer checks want 16-byte alignment)


def rejected(lib, rc, *words):
    msg = lib.ptk_last_error()
    return rc == -1 and all(w in msg for w in words)


def test_symbols_exported_and_bound(env):
    L, lib, _, _ = env
    for name in NEW:
        assert name in L.SIGNATURES and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert lib.ptk_abi_version() == L.ABI_VERSION == 8
    from projectiontrainer_amd import kernels as Kn
    for name in ("gemm_row_stats", "cross_entropy_stats_", "count_valid", "loss_reduce"):
        assert callable(getattr(Kn, name))


def _desc(L, p, **kw):
    """A descriptor ptk_gemm_row_stats accepts (M 64, N 128, K 64), with the fields of kw changed."""
    d = L.GemmDesc()
    d.A, d.B, d.C = p, p, p
    d.M, d.N, d.K = 64, 128, 64
    d.lda, d.ldb, d.ldc = 64, 64, 128
    d.batch, d.batch_inner = 1, 1
    d.alpha, d.act, d.out = 1.0, L.ACT_NONE, L.OUT_BF16
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_gemm_row_stats_refuses_what_the_epilogue_would_not_honour(env):
    L, lib, buf, p = env
    call = lambda stats=p, ld_stats=4, **kw: lib.ptk_gemm_row_stats(_desc(L, p, **kw), stats, ld_stats, None)
    assert rejected(lib, lib.ptk_gemm_row_stats(None, p, 4, None), b"desc")
    for act in (L.ACT_GELU_TANH, L.ACT_GELU_ERF, L.ACT_GEGLU, L.ACT_GELU_ERF_BWD, L.ACT_GEGLU_BWD):
        assert rejected(lib, call(act=act), b"row_stats", b"act"), act
    for out in (L.OUT_F32, L.OUT_F32_BF16ROUND):
        assert rejected(lib, call(out=out), b"row_stats", b"out"), out
    assert rejected(lib, call(batch=2), b"row_stats", b"batch")
    for N in (8, 96, 100, 136):
        assert rejected(lib, call(N=N, ldc=136), b"row_stats", b"N ", str(N).encode()), N
    for ldc in (132, 120, 64, 129):                       # ldc % 8, ldc < N
        assert rejected(lib, call(ldc=ldc), b"row_stats", b"ldc", str(ldc).encode()), ldc
    assert rejected(lib, call(C=p + 8), b"row_stats", b"C ", b"aligned")
    for field in ("bias", "rowadd", "resid", "resid16", "aux", "aux2", "aux_in", "aux_in2"):
        word = field.rstrip("2").encode()
        assert rejected(lib, call(**{field: p}), b"row_stats", word), field
    for cmap in (L.RowMap(4, 0, 8, 0), L.RowMap(0, 0, 0, 2), L.RowMap(4, 1, 4, 0), L.RowMap(0, 0, 0, -1)):
        assert rejected(lib, call(cmap=cmap), b"row_stats", b"cmap")
    for alpha in (0.5, 2.0, 0.0):
        assert rejected(lib, call(alpha=alpha), b"row_stats", b"alpha"), alpha
    for flag in ("A_kt", "C_kt", "aux_kt", "aux_in_kt"):
        assert call(**{flag: 1}) == -1, flag
    for ld_stats in (2, 3, 5, 0, -4):                     # < 2 N / 64, odd
        assert rejected(lib, call(ld_stats=ld_stats), b"row_stats", b"ld_stats", str(ld_stats).encode()), ld_stats
    assert rejected(lib, call(stats=None), b"stats", b"NULL")
    assert rejected(lib, call(stats=p + 4), b"row_stats", b"stats", b"aligned")
    for field in ("A", "B", "C"):
        assert rejected(lib, call(**{field: None}), b"NULL"), field
    # the plain GEMM's own rules still come first
    assert rejected(lib, call(K=60), b"multiple of 64")
    # nothing to do: no launch, no error
    assert call(M=0) == 0
    assert bytes(buf) == b"\x5a" * 4096


def test_cross_entropy_stats_refusals(env):
    L, lib, buf, p = env
    ce = lambda ld=136, rows=4, vocab=128, stats=p, ld_stats=4, logits=p, tgt=p, rl=p, gs=p: \
        lib.ptk_cross_entropy_stats(logits, ld, rows, vocab, stats, ld_stats, tgt, rl, gs, None)
    for vocab in (8, 100, 2056, 14344, 0, -64):
        assert rejected(lib, ce(vocab=vocab, ld=14400, ld_stats=1000), b"vocab", str(vocab).encode()), vocab
    for ld in (132, 129, 120, 64):                        # ld % 8, ld < vocab
        assert rejected(lib, ce(ld=ld), b"ld ", str(ld).encode()), ld
    for ld_stats in (2, 3, 0, -2):
        assert rejected(lib, ce(ld_stats=ld_stats), b"ld_stats", str(ld_stats).encode()), ld_stats
    assert rejected(lib, ce(ld_stats=5), b"ld_stats")     # odd: the float2 loads would be misaligned
    assert ce(rows=0) == 0 and ce(rows=-3) == 0
    for name in ("logits", "stats", "tgt", "rl", "gs"):
        assert rejected(lib, ce(**{name: None}), b"NULL"), name
    assert rejected(lib, ce(logits=p + 8), b"aligned") and rejected(lib, ce(stats=p + 4), b"aligned")
    assert bytes(buf) == b"\x5a" * 4096


def test_count_valid_and_loss_reduce_refuse_null(env):
    L, lib, buf, p = env
    assert rejected(lib, lib.ptk_count_valid(None, 4, 1.0, p, p, None), b"NULL", b"labels")
    assert rejected(lib, lib.ptk_count_valid(p, 4, 1.0, None, p, None), b"NULL", b"gscale")
    assert rejected(lib, lib.ptk_count_valid(p, 4, 1.0, p, None, None), b"NULL", b"count")
    assert rejected(lib, lib.ptk_count_valid(p, 0, 1.0, None, p, None), b"NULL")        # outputs are written at n = 0
    assert rejected(lib, lib.ptk_loss_reduce(None, 4, p, p, None), b"NULL", b"row_loss")
    assert rejected(lib, lib.ptk_loss_reduce(p, 4, None, p, None), b"NULL", b"count")
    assert rejected(lib, lib.ptk_loss_reduce(p, 4, p, None, None), b"NULL", b"loss")
    assert rejected(lib, lib.ptk_loss_reduce(p, 0, p, None, None), b"NULL")
    assert bytes(buf) == b"\x5a" * 4096


# ---------------------------------------------------------------- the fp64 helpers
def _small_case():
    g = torch.Generator().manual_seed(11)
    logits = (torch.randn(9, 192, generator=g) * 4).bfloat16()
    logits[3] *= 40                                         # |x| in the hundreds
    tgt = torch.tensor([0, 191, 63, 64, U.IGNORE, 7, 130, U.IGNORE, 100])
    return logits, tgt


def test_fp64_helpers_agree_with_torch_fp64():
    logits, tgt = _small_case()
    x = logits.double()
    torch.testing.assert_close(U.lse_ref(logits), torch.logsumexp(x, dim=-1), rtol=1e-14, atol=1e-13)
    want = F.cross_entropy(x, tgt, reduction="none", ignore_index=U.IGNORE)
    got = U.row_loss_ref(logits, tgt)
    torch.testing.assert_close(got, want, rtol=1e-13, atol=1e-12)
    assert torch.equal(got[tgt < 0], torch.zeros(2, dtype=torch.float64))
    # chunk statistics recombine to the row's log-sum-exp
    m, s = U.chunk_stats_ref(logits)
    assert m.shape == s.shape == (9, 3)
    assert torch.equal(m, x.view(9, 3, 64).amax(dim=-1))
    torch.testing.assert_close(torch.logsumexp(m + torch.log(s), dim=-1), U.lse_ref(logits), rtol=1e-14, atol=1e-13)
    # d(logits): autograd of the summed loss times g, in fp64; ignored rows exactly zero
    g = 0.25 / 7
    xr = x.clone().requires_grad_(True)
    (F.cross_entropy(xr, tgt, reduction="sum", ignore_index=U.IGNORE) * g).backward()
    exact, weight = U.dlogits_ref(logits, tgt, g)
    torch.testing.assert_close(exact, xr.grad, rtol=1e-12, atol=1e-18)
    assert not exact[tgt < 0].any() and not weight[tgt < 0].any()
    assert torch.equal(weight[0, 0], torch.softmax(x[0], -1)[0] + 1)
    # an all -inf chunk: (max -inf, sum NaN); the row stays finite
    logits[5, 64:128] = float("-inf")
    m, s = U.chunk_stats_ref(logits)
    assert m[5, 1] == float("-inf") and torch.isnan(s[5, 1]) and torch.isfinite(U.lse_ref(logits)).all()


def test_ulp_helpers():
    x = torch.tensor([1.0, 1.5, 2.0, 0.75, -3.0, 2.0 ** -126, 2.0 ** -130, 0.0, 300.0], dtype=torch.float64)
    assert U.ulp_bf16(x).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -6, 2.0 ** -133, 2.0 ** -133,
                                      2.0 ** -133, 2.0]
    assert U.ulp32(x).tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -24, 2.0 ** -22, 2.0 ** -149,
                                   2.0 ** -149, 2.0 ** -149, 2.0 ** -15]
    # against the formats themselves: the gap to the next representable number
    for v in (1.0, 0.37, 513.0, 1e-3):
        b = torch.tensor(v).bfloat16()
        nxt = (U.bits(b) + 1).view(torch.bfloat16)
        assert float(nxt.double() - b.double()) == float(U.ulp_bf16(b.double()))
        f = torch.tensor(v, dtype=torch.float32)
        assert float(torch.nextafter(f, torch.tensor(float("inf"))).double() - f.double()) == float(U.ulp32(f.double()))


@pytest.mark.parametrize("K", [64, 128])
def test_exact_operands_give_fp32_exact_products(K):
    """Every partial sum is an fp32 number: the fp32 product in any order equals the fp64 one, also over the scaled
    rows, and the scaled rows do what they are for."""
    A, B = U.exact_operands(40, 192, K, seed=3, big_rows=(1, 7), small_rows=(2, 9))
    P, L16 = U.exact_logits(A, B)
    a32, b32 = A.float(), B.float()
    assert torch.equal((a32 @ b32.T).double(), P)
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(1))
    assert torch.equal((a32[:, perm] @ b32[:, perm].T).double(), P)
    acc = torch.zeros(40, 192)
    for k in reversed(range(K)):                            # one term at a time, back to front
        acc += a32[:, k:k + 1] * b32[:, k].unsqueeze(0)
    assert torch.equal(acc.double(), P)
    vals = torch.cat([A[[0, 3, 4]].double().flatten(), B.double().flatten()])
    assert vals.abs().max() <= 2 and torch.equal(vals * 8, (vals * 8).round())
    assert P[[1, 7]].abs().max() > 100                      # exp() of these overflows fp32 without the max shift
    assert float(torch.exp(P[[1, 7]].max().float())) == float("inf")
    small = L16[[2, 9]].double()
    assert float((small.amax(dim=-1) - small.amin(dim=-1)).max()) < 20      # crowded: every column counts in the sum
    assert all(len(torch.unique(r)) < r.numel() for r in small)              # and columns tie after the bf16 rounding
    assert torch.equal(L16.double(), U.bf16_rne(P).double())
