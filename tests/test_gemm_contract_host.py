"""launch_gemm's validation (csrc/gemm.hip epilogue_check, stated next to ptk_gemm_desc in include/ptk.h): every
descriptor an epilogue could not honour bit for bit is refused before any device call, so the refusals hold without a
GPU.  Host memory stands in for the device buffers and must come back untouched.  Every descriptor this
file sends is refused, or (M or N zero) returns 0 on launch_gemm's first line: none reaches a device call (the pattern
of tests/test_loss_head_host.py)."""
import ctypes

import pytest

from tests import gemm_ref as G

FILL = 0x5A


@pytest.fixture(scope="module")
def env():
    from projectiontrainer_amd import _lib as L
    buf = (ctypes.c_char * 8192)(*([FILL] * 8192))
    return L, L.lib(), buf, (ctypes.addressof(buf) + 63) & ~63


def _desc(L, p, **kw):
    """A plain descriptor ptk_gemm would launch (M 64, N 128, K 64, packed), with the fields of kw changed."""
    d = L.GemmDesc()
    d.A, d.B, d.C = p, p, p
    d.M, d.N, d.K = 64, 128, 64
    d.lda, d.ldb, d.ldc = 64, 64, 128
    d.batch, d.batch_inner = 1, 1
    d.alpha, d.act, d.out = 1.0, L.ACT_NONE, L.OUT_BF16
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _refused(lib, rc, *words):
    msg = lib.ptk_last_error()
    return rc == -1 and all(w in msg for w in words)


def _geglu(p, **kw):       # an acceptable GEGLU descriptor: C [64, 64], aux / aux2 [64, 64]
    return dict(dict(act=G.ACT_GEGLU, ldc=64, aux=p, aux2=p, ld_aux=64), **kw)


def _geglu_bwd(p, **kw):   # an acceptable GEGLU-backward descriptor: C [64, 256], aux_in / aux_in2 [64, 128]
    return dict(dict(act=G.ACT_GEGLU_BWD, ldc=256, aux_in=p, aux_in2=p, ld_aux_in=128), **kw)


@pytest.mark.parametrize("mode", G.MODES)
def test_refusals_under_every_force_mode(env, mode):
    """No force mode routes a refused descriptor to a kernel: the check runs before the planner."""
    L, lib, buf, p = env
    call = lambda **kw: lib.ptk_gemm(_desc(L, p, **kw), None)
    L.check(lib.ptk_gemm_force_small_tiles(mode), "force")
    try:
        # saved inputs the backward epilogues dereference unconditionally
        assert _refused(lib, call(act=G.ACT_GELU_ERF_BWD), b"aux_in")
        assert _refused(lib, call(act=G.ACT_GELU_ERF_BWD, aux_in2=p, ld_aux_in=128), b"aux_in")
        assert _refused(lib, call(**_geglu_bwd(p, aux_in=None)), b"aux_in")
        assert _refused(lib, call(**_geglu_bwd(p, aux_in2=None)), b"aux_in2")
        assert _refused(lib, call(act=G.ACT_GEGLU_BWD, ldc=256), b"aux_in")
        # partial interleave groups: columns would be dropped
        for N in (8, 16, 48, 100, 130, 144):
            assert _refused(lib, call(**_geglu(p, N=N, ldc=128)), b"GEGLU", b"32"), N
        for N in (4, 8, 24, 100, 130, 136):
            assert _refused(lib, call(**_geglu_bwd(p, N=N, ldc=512, ld_aux_in=256)), b"GEGLU", b"16"), N
        # leading dimensions the 8-byte GEGLU accesses cannot take
        for ldc in (65, 66, 67, 70):
            assert _refused(lib, call(**_geglu(p, ldc=ldc)), b"ldc", str(ldc).encode()), ldc
        for ld in (65, 66, 67, 70):
            assert _refused(lib, call(**_geglu(p, ld_aux=ld)), b"ld_aux", str(ld).encode()), ld
            assert _refused(lib, call(**_geglu(p, ld_aux=ld, aux=None)), b"ld_aux"), ld     # aux2 alone
        for ldc in (257, 258, 259, 262):
            assert _refused(lib, call(**_geglu_bwd(p, ldc=ldc)), b"ldc", str(ldc).encode()), ldc
        for ld in (129, 130, 131, 134):
            assert _refused(lib, call(**_geglu_bwd(p, ld_aux_in=ld)), b"ld_aux_in", str(ld).encode()), ld
        # inputs the GEGLU epilogues never read
        for field, extra in (("bias", {}), ("rowadd", dict(rowadd_period=4, ld_rowadd=128)),
                             ("resid", dict(ld_resid=128)), ("resid16", dict(ld_resid16=128))):
            assert _refused(lib, call(**_geglu(p, **{field: p}, **extra)), b"GEGLU", field.encode()), field
            assert _refused(lib, call(**_geglu_bwd(p, **{field: p}, **extra)), b"GEGLU", field.encode()), field
        assert _refused(lib, call(**_geglu(p, bf16_linear=1)), b"bf16_linear")
        assert _refused(lib, call(**_geglu_bwd(p, bf16_linear=1)), b"bf16_linear")
        # the row-add table's period is a divisor
        for period in (0, -1, -37):
            assert _refused(lib, call(rowadd=p, rowadd_period=period, ld_rowadd=128), b"rowadd_period"), period
        assert _refused(lib, call(amap=L.RowMap(8, 1, 8, 0)), b"amap.skip")        # (a dropped A row has no address)
        for field in ("A", "B", "C"):
            assert _refused(lib, call(**{field: None}), b"NULL"), field
        # the rules that were there before still hold
        assert _refused(lib, call(K=60), b"multiple of 64")
        assert _refused(lib, call(lda=68), b"lda")
        assert _refused(lib, call(act=G.ACT_GELU_TANH, aux=p, ld_aux=136), b"ld_aux == ldc")
        assert _refused(lib, call(act=G.ACT_GELU_TANH, aux=p, ld_aux=128, cmap=L.RowMap(0, 0, 0, 8)), b"identity")
        assert _refused(lib, call(act=G.ACT_GELU_ERF, out=L.OUT_F32), b"unsupported")
        assert lib.ptk_gemm(None, None) == -1
        # nothing to do: no launch, no error
        assert call(M=0) == 0 and call(N=0, act=G.ACT_GELU_ERF_BWD) == 0
    finally:
        lib.ptk_gemm_force_small_tiles(0)
    assert bytes(buf) == bytes([FILL]) * 8192


def test_act_constants_match_the_library():
    from projectiontrainer_amd import _lib as L
    assert (L.ACT_NONE, L.ACT_GELU_TANH, L.ACT_GELU_ERF, L.ACT_GEGLU, L.ACT_GELU_ERF_BWD, L.ACT_GEGLU_BWD) == tuple(range(6))
    assert (L.OUT_BF16, L.OUT_F32, L.OUT_F32_BF16ROUND) == (0, 1, 2)
    assert len(G.ACT_NAMES) == 6
