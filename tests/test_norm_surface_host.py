"""The unit-test surface of the Gemma3 norm kernels and the norm weight-grad block (include/ptk.h): exported and bound,
and its argument validation, which runs before any device call and so holds without a GPU.  Host memory stands in for
the device buffers and must come back untouched."""
import ctypes

import pytest

NEW = ["ptk_residual_norm_fwd", "ptk_residual_norm_bwd_partial_floats", "ptk_residual_norm_bwd", "ptk_post_norm_bwd",
       "ptk_rmsnorm_bwd_bdn", "ptk_rmsnorm_mapped", "ptk_rmsnorm_bwd_scatter", "ptk_rms_wgrad_partial_floats",
       "ptk_rms_wgrad", "ptk_rms_wgrad_finish_floats", "ptk_rms_wgrad_finish", "ptk_qknorm_wgrad_partial_floats",
       "ptk_qknorm_wgrad"]
F32, BF16, WG_FUSED, WG_SPLIT = range(4)
BAD_COLS = (0, 1154, 3076)      # the norm launchers' rule: a multiple of 4, 1 .. 3072


@pytest.fixture(scope="module")
def env():
    from projectiontrainer_amd import _lib as L
    buf = (ctypes.c_char * 4096)(*([0x5A] * 4096))
    return L, L.lib(), buf, ctypes.addressof(buf)


def rejected(lib, rc, *words):
    msg = lib.ptk_last_error()
    return rc == -1 and all(w in msg for w in words)


def test_symbols_exported_and_bound(env):
    L, lib, _, _ = env
    for name in NEW:
        assert name in L.SIGNATURES and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert lib.ptk_abi_version() == 8


def test_norm_entries_reject_bad_cols_and_null(env):
    L, lib, buf, p = env
    ident = L.RowMap(0, 0, 0, 0)
    calls = {
        "residual_norm_fwd": lambda rows, cols, a=p: lib.ptk_residual_norm_fwd(a, p, p, p, p, p, p, p, rows, cols, 1e-6, None),
        "post_norm_bwd": lambda rows, cols, a=p: lib.ptk_post_norm_bwd(a, p, p, p, p, rows, cols, None),
        "rmsnorm_bwd_bdn": lambda rows, cols, a=p: lib.ptk_rmsnorm_bwd_bdn(a, p, p, p, None, p, rows, cols, None),
        "rmsnorm_mapped": lambda rows, cols, a=p: lib.ptk_rmsnorm_mapped(a, max(cols, 4), ident, p, p, p, rows, cols, 1e-6, None),
        "rmsnorm_bwd_scatter": lambda rows, cols, a=p: lib.ptk_rmsnorm_bwd_scatter(a, ident, p, p, p, p, rows, cols, None),
    }
    for mode in (F32, BF16, WG_FUSED, WG_SPLIT):
        calls[f"residual_norm_bwd mode {mode}"] = \
            lambda rows, cols, a=p, m=mode: lib.ptk_residual_norm_bwd(m, a, p, p, p, p, p, p, p, p, rows, cols, p, p, p,
                                                                      1 << 40, None)
    for name, call in calls.items():
        for cols in BAD_COLS:
            assert rejected(lib, call(4, cols), b"cols", str(cols).encode()), (name, cols)
        assert call(0, 1152) == 0 and call(-3, 4) == 0, name                   # no rows: nothing to do
        assert rejected(lib, call(4, 1152, None), b"NULL"), name
    # w_next given without n / rstd_x; w_next NULL needs neither
    assert rejected(lib, lib.ptk_residual_norm_fwd(p, p, p, p, p, None, p, p, 4, 8, 1e-6, None), b"NULL")
    assert rejected(lib, lib.ptk_residual_norm_bwd(7, p, p, p, p, p, p, p, p, p, 4, 8, p, p, p, 64, None), b"mode")
    # weight-grad modes: both grads and the partial buffer, of the stated size
    for mode in (WG_FUSED, WG_SPLIT):
        need = lib.ptk_residual_norm_bwd_partial_floats(37, 1152, mode)
        assert need > 0
        assert rejected(lib, lib.ptk_residual_norm_bwd(mode, p, p, p, p, p, p, p, p, p, 37, 1152, p, p, p, need - 1,
                                                       None), b"partial")
        assert rejected(lib, lib.ptk_residual_norm_bwd(mode, p, p, p, p, p, p, p, p, p, 37, 1152, p, None, p, need,
                                                       None), b"NULL")
    # row maps that would drop rows, and a leading dimension below cols or off the 16-byte loads
    skip = L.RowMap(4, 1, 8, 0)
    assert rejected(lib, lib.ptk_rmsnorm_mapped(p, 8, skip, p, p, p, 4, 8, 1e-6, None), b"row map")
    assert rejected(lib, lib.ptk_rmsnorm_bwd_scatter(p, skip, p, p, p, p, 4, 8, None), b"row map")
    assert rejected(lib, lib.ptk_rmsnorm_mapped(p, 4, ident, p, p, p, 4, 8, 1e-6, None), b"ldx")
    assert rejected(lib, lib.ptk_rmsnorm_mapped(p, 10, ident, p, p, p, 4, 8, 1e-6, None), b"ldx")
    assert bytes(buf) == b"\x5a" * 4096


def test_wgrad_entries_reject_before_any_launch(env):
    L, lib, buf, p = env
    ident = L.RowMap(0, 0, 0, 0)
    wg = lambda cols, rows=4, xb=0, db=0, rnd=0, ldx=None, lddy=None, pf=1 << 40, m=ident, x=p: lib.ptk_rms_wgrad(
        x, xb, cols + 4 if ldx is None else ldx, m, p, p, db, cols + 4 if lddy is None else lddy, rnd, rows, cols, p, p,
        pf, None)
    for cols in (0, 1154, 4100, -4):
        assert rejected(lib, wg(cols), b"cols"), cols
    assert wg(4096, rows=0) == 0 and wg(8, rows=-1) == 0
    assert rejected(lib, wg(8, xb=1, db=1), b"bf16")                       # not an instantiated pair
    assert rejected(lib, wg(8, db=1, rnd=1), b"dy_round")
    assert rejected(lib, wg(8, ldx=4), b"ldx") and rejected(lib, wg(8, lddy=10), b"lddy")
    assert rejected(lib, wg(8, m=L.RowMap(4, 2, 8, 0)), b"row map")
    assert rejected(lib, wg(8, x=None), b"NULL")
    assert rejected(lib, wg(1152, rows=130, pf=lib.ptk_rms_wgrad_partial_floats(130, 1152) - 1), b"partial")
    # the fold alone
    fin = lambda nblk, cols, pf=1 << 40, part=p: lib.ptk_rms_wgrad_finish(part, nblk, cols, p, pf, None)
    assert rejected(lib, fin(4, 0), b"cols") and rejected(lib, fin(4, 4097), b"cols")
    assert fin(0, 64) == 0 and fin(-2, 64) == 0
    assert rejected(lib, fin(4, 64, part=None), b"NULL")
    assert rejected(lib, fin(257, 100, pf=lib.ptk_rms_wgrad_finish_floats(257, 100) - 1), b"partial")
    # q/k norm grads: head_dim a multiple of 8 up to 256
    qk = lambda D, B=3, S=37, Hq=4, Hkv=1, pf=1 << 40, q=p: lib.ptk_qknorm_wgrad(q, p, p, B, S, Hq, Hkv, D, p, p, p, p, p,
                                                                              p, p, pf, None)
    for D in (264, 12, 0):
        assert rejected(lib, qk(D), b"head_dim", str(D).encode()), D
    assert rejected(lib, qk(64, Hq=4, Hkv=3), b"heads")
    assert qk(64, B=0) == 0 and qk(64, S=0) == 0
    assert rejected(lib, qk(64, q=None), b"NULL")
    assert rejected(lib, qk(256, pf=lib.ptk_qknorm_wgrad_partial_floats(111, 256) - 1), b"partial")
    assert bytes(buf) == b"\x5a" * 4096


def test_size_functions_match_the_launchers_formulas(env):
    """ptk_internal.h / train.hip / norm.hip: 32-row partial blocks and one 16-row fold behind them; the fused
    backward writes one partial row per 4-row block, twice; 8 token rows per q/k block, two sets and one fold."""
    _, lib, _, _ = env
    fold = lambda nblk: nblk + (nblk + 15) // 16
    for cols in (4, 100, 1152, 4096):
        prev = 0
        for nblk in (1, 15, 16, 17, 256, 257, 4097):
            got = lib.ptk_rms_wgrad_finish_floats(nblk, cols)
            assert got == fold(nblk) * cols and got > prev
            prev = got
    for cols in (4, 1152, 3072):
        prev = [0, 0, 0]
        for rows in (1, 4, 5, 31, 32, 33, 130, 8225, 14336):
            got = [lib.ptk_rms_wgrad_partial_floats(rows, cols),
                   lib.ptk_residual_norm_bwd_partial_floats(rows, cols, WG_FUSED),
                   lib.ptk_residual_norm_bwd_partial_floats(rows, cols, WG_SPLIT)]
            assert got[0] == fold((rows + 31) // 32) * cols
            assert got[1] == 2 * fold((rows + 3) // 4) * cols
            assert got[2] == got[0]
            assert all(g >= q for g, q in zip(got, prev))                  # monotone in rows
            prev = got
            assert lib.ptk_residual_norm_bwd_partial_floats(rows, cols, F32) == 0
            assert lib.ptk_residual_norm_bwd_partial_floats(rows, cols, BF16) == 0
    for D in (8, 64, 256):
        prev = 0
        for M in (1, 8, 9, 111, 2060):
            got = lib.ptk_qknorm_wgrad_partial_floats(M, D)
            nblk = (M + 7) // 8
            assert got == (2 * nblk + (nblk + 15) // 16) * D and got >= prev
            prev = got
    assert lib.ptk_rms_wgrad_partial_floats(0, 64) == 0 and lib.ptk_rms_wgrad_finish_floats(0, 64) == 0
    assert lib.ptk_qknorm_wgrad_partial_floats(0, 64) == 0
    # past the surface's limits: no size
    assert lib.ptk_rms_wgrad_partial_floats((1 << 20) + 1, 64) == -1
    assert lib.ptk_residual_norm_bwd_partial_floats((1 << 20) + 1, 64, WG_FUSED) == -1
