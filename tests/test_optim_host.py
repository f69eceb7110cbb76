"""Argument validation of the optimizer and embedding-gradient entry points.  It runs before any launch, so it holds
without a GPU: host memory stands in for the device buffers and must come back untouched."""
import ctypes

NV = 3


def host_buffers(n, H=8, vocab=4):
    """Host memory stands in for the device buffers: every call below must return before any launch."""
    ids = (ctypes.c_int64 * max(n, 1))()
    dx = (ctypes.c_float * 64)()
    dE = (ctypes.c_uint16 * (vocab * H))(*([0x3F80] * (vocab * H)))
    ws = (ctypes.c_uint64 * max(n, 1))()
    return ids, dx, dE, ws


def test_embed_grad_argument_checks_need_no_gpu():
    """n = 0 returns 0 and touches nothing; 16 385 tokens (one past the 14-bit position of a sort key) and a
    workspace one byte short are errors before any launch."""
    from projectiontrainer_amd import _lib as L
    lib = L.lib()
    A = ctypes.addressof
    assert lib.ptk_embed_grad_workspace_bytes(4, 5) >= 4 * 5 * 8
    ids, dx, dE, ws = host_buffers(4)
    assert lib.ptk_embed_grad(A(ids), 0, 4, NV, 12, 8, 1.0, A(dx), A(dE), A(ws), 32, None) == 0
    assert lib.ptk_embed_grad(A(ids), 4, 0, NV, 8, 8, 1.0, A(dx), A(dE), A(ws), 32, None) == 0
    assert list(dE) == [0x3F80] * 32
    big = (ctypes.c_uint64 * 16385)()
    bigids = (ctypes.c_int64 * 16385)()
    rc = lib.ptk_embed_grad(A(bigids), 1, 16385, NV, 16385 + 8, 8, 1.0, A(dx), A(dE), A(big), 16385 * 8, None)
    assert rc != 0 and b"16385" in lib.ptk_last_error() and b"max" in lib.ptk_last_error()
    rc = lib.ptk_embed_grad(A(bigids), 5, 3277, NV, 3277 + 8, 8, 1.0, A(dx), A(dE), A(big), 16385 * 8, None)
    assert rc != 0 and b"16385" in lib.ptk_last_error()
    need = lib.ptk_embed_grad_workspace_bytes(1, 4)
    rc = lib.ptk_embed_grad(A(ids), 1, 4, NV, 12, 8, 1.0, A(dx), A(dE), A(ws), need - 1, None)
    assert rc != 0 and b"workspace" in lib.ptk_last_error()
    rc = lib.ptk_embed_grad(A(ids), 1, 4, NV, 6, 8, 1.0, A(dx), A(dE), A(ws), need, None)     # rows would overlap
    assert rc != 0 and b"seq_pad" in lib.ptk_last_error()
    rc = lib.ptk_embed_grad(None, 1, 4, NV, 12, 8, 1.0, A(dx), A(dE), A(ws), need, None)
    assert rc != 0 and b"NULL" in lib.ptk_last_error()
    assert list(dE) == [0x3F80] * 32 and not any(ws)


def test_optimizer_alignment_checks_need_no_gpu():
    """ptk_bf16_grad_scale_sumsq loads g, and ptk_clip_adamw's norm pass loads grads, 16 bytes at a time
    (include/ptk.h): a pointer off that alignment is an error before any launch."""
    from projectiontrainer_amd import _lib as L
    lib = L.lib()
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 15) & ~15
    part, out = base + 1024, base + 2048
    for off in (2, 4, 8, 14):
        rc = lib.ptk_bf16_grad_scale_sumsq(base + off, 16, 0.5, part, out, None)
        assert rc != 0 and b"16-byte aligned" in lib.ptk_last_error()
    for off in (4, 8, 12):
        rc = lib.ptk_clip_adamw(base + 256, base + 512 + off, base + 768, base + 1280, 16, 1.0, 5.0, 1e-3, 0.9, 0.999,
                                1e-8, 0.01, 1, part, out, None)
        assert rc != 0 and b"16-byte aligned" in lib.ptk_last_error()
    assert bytes(buf) == bytes(4096)
