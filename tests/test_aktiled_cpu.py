"""k-step-tiled activations, the host side (no GPU): the producer / consumer pair predicate
(ptk_gemm_ktiled_pair, gemm_plan.cpp gemm_ktiled_pair) at the cfg2 Gemma MLP shapes and with each of its conditions
violated in turn, and the layout's un-tiling index (tests/ktiled_util.py) against ptk_kstep_tile_offset."""
import numpy as np
import pytest

from tests.ktiled_util import tiled_source_index

NCU = 256
M1, H, I = 22528, 1152, 6912   # cfg2: 32 x 704 token rows, Gemma3-1B widths
BIG = 1 << 28                  # fp32 scratch floats offered to the consumer's K split (ample)


def _lib():
    from projectiontrainer_amd import _lib as L
    return L


def desc(L, M, N, K, act, A, C, ldc, **kw):
    d = L.GemmDesc()
    d.A, d.B, d.C, d.B_kt = A, 0x10000000, C, 0x20000000
    d.M, d.N, d.K, d.lda, d.ldb, d.ldc = M, N, K, K, K, ldc
    d.alpha, d.act, d.out, d.batch, d.batch_inner = 1.0, act, L.OUT_BF16, 1, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def fwd_pair(L, M=M1, N=2 * I, **kw):
    """gate|up (GEGLU, h [M, N / 2] with the factors beside it) -> down"""
    p = desc(L, M, N, H, L.ACT_GEGLU, 0x30000000, 0x40000000, N // 2, aux=0x50000000, aux2=0x60000000, ld_aux=N // 2,
             **kw)
    return p, desc(L, M, H, N // 2, L.ACT_NONE, 0x40000000, 0x70000000, H)


def bwd_pair(L, M=M1, N=I, **kw):
    """dh (GEGLU backward, dg | du [M, 2 N], the factors read) -> d(gate|up) dX"""
    p = desc(L, M, N, H, L.ACT_GEGLU_BWD, 0x30000000, 0x40000000, 2 * N, aux_in=0x50000000, aux_in2=0x60000000,
             ld_aux_in=N, **kw)
    return p, desc(L, M, H, 2 * N, L.ACT_NONE, 0x40000000, 0x70000000, H)


def pair(L, pc, part=BIG, train=0):
    return L.lib().ptk_gemm_ktiled_pair(pc[0], pc[1], NCU, part, train)


def test_pair_yes_at_cfg2_shapes():
    L = _lib()
    assert pair(L, fwd_pair(L)) == 1
    assert pair(L, bwd_pair(L)) == 1


@pytest.mark.parametrize("mk", [fwd_pair, bwd_pair])
def test_pair_no_per_violated_condition(mk, monkeypatch):
    L = _lib()
    assert pair(L, mk(L)) == 1
    assert pair(L, mk(L, M=22520)) == 0                                  # M % 16
    assert pair(L, mk(L, cmap=L.RowMap(16, 0, 32, 0))) == 0              # a row map on C
    assert pair(L, mk(L, cmap=L.RowMap(0, 0, 0, 8))) == 0                # a row offset that is not 16-aligned
    assert pair(L, mk(L, batch=2)) == 0                                  # batch 2
    assert pair(L, mk(L), train=1) == 0                                  # Stage 2
    p, c = mk(L)
    p.ldc += 64
    assert pair(L, (p, c)) == 0                                          # C not packed
    p, c = mk(L)
    p.B_kt = None
    assert pair(L, (p, c)) == 0                                          # the variants stream a tiled B
    # a consumer whose plan is not the 8-wave kernel: force mode 8 plans every launch onto the 4-wave one
    L.lib().ptk_gemm_force_small_tiles(8)
    try:
        assert pair(L, mk(L)) == 0
    finally:
        L.lib().ptk_gemm_force_small_tiles(0)
    monkeypatch.setenv("PTK_A_KTILED", "0")                              # the switch
    assert L.lib().ptk_a_ktiled_reload() == 0
    try:
        assert pair(L, mk(L)) == 0
    finally:
        monkeypatch.delenv("PTK_A_KTILED")
        assert L.lib().ptk_a_ktiled_reload() == 1
    assert pair(L, mk(L)) == 1


def test_pair_no_for_geglu_width_of_half_k_steps():
    """N % 64 != 0: h's width N / 2 is not whole k-steps."""
    L = _lib()
    assert pair(L, fwd_pair(L, N=2 * I + 32)) == 0


def test_pair_no_when_the_consumer_is_k_split():
    """Stage 2's down projection at M = 14 336 (280 tiles) with scratch for two slices' partials but not for the
    stream-K slabs: gemm_split_plan cuts it along K, and a K slice cannot read a tiled A.  With the slabs' worth of
    scratch the split plan lends it to the stream-K tail instead: no either way."""
    L = _lib()
    M = 14336
    p, c = fwd_pair(L, M=M)
    part = 2 * M * H
    sl, kc = L.C.c_int(), L.C.c_int()
    assert L.lib().ptk_gemm_split_plan(c, NCU, part, L.C.byref(sl), L.C.byref(kc), None, None) == 0
    assert sl.value == 2 and kc.value == I // 2
    assert pair(L, (p, c), part=part) == 0
    tw = L.C.c_int()
    assert L.lib().ptk_gemm_split_plan(c, NCU, BIG, L.C.byref(sl), L.C.byref(kc), None, L.C.byref(tw)) == 0
    assert kc.value == 0 and tw.value == 1
    assert pair(L, (p, c), part=BIG) == 0
    assert pair(L, (p, c), part=0) == 1   # (no scratch: unsplit on 224-row tiles)


@pytest.mark.parametrize("M,K", [(16, 32), (48, 160), (320, 1152)])
def test_untiling_index_round_trips(M, K):
    L = _lib()
    idx = tiled_source_index(M, K)
    assert np.array_equal(np.sort(idx), np.arange(M * K))
    x = np.random.default_rng(M + K).integers(0, 1 << 16, M * K).astype(np.uint16)
    tiled = x[idx]
    back = np.empty_like(x)
    back[idx] = tiled
    assert np.array_equal(back, x)
    off = L.lib().ptk_kstep_tile_offset
    for row, k in ((0, 0), (M - 1, K - 1), (M // 2 + 3, K // 2 + 5), (7, 31), (15, 8)):
        j = off(row, k, K) // 2
        assert idx[j] == row * K + k
