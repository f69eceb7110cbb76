"""Argument validation of the repetition-penalty entry points (ptk_sample_next_token, ptk_beam_candidates_penalized,
ptk_gemma3_generate_penalized).  It runs before any device call, so it holds without a GPU: host memory stands in
for the device buffers and must come back untouched.  The rule for the penalty is HF's (a float > 0), finite as
well; a history must be present when n_hist > 0, with history_ld >= n_hist; top-k + history must fit the LDS
lists.  The ABI version does not move: the entry points are additions."""
import ctypes

import pytest

V, B, K, NC = 64, 2, 3, 6
A = ctypes.addressof


def _buffers():
    return dict(logits=(ctypes.c_uint16 * (B * K * V))(), scores=(ctypes.c_float * (B * K))(),
                hist=(ctypes.c_int64 * (B * K * 2048))(), tok=(ctypes.c_int64 * (B * NC))(),
                beam=(ctypes.c_int32 * (B * NC))(), out=(ctypes.c_float * (B * NC))(),
                ws=(ctypes.c_char * 8192)())


def _sample(lib, b, hist, ld, n_hist, p, do_sample=0, top_k=0):
    return lib.ptk_sample_next_token(A(b["logits"]), V, B, V, do_sample, top_k, 1.0, 1.0, 0, 0, -1, 0, None, hist, ld,
                                     n_hist, p, A(b["tok"]), A(b["ws"]), 8192, None)


def _beam(lib, b, hist, ld, n_hist, p, do_sample=0, top_k=0):
    return lib.ptk_beam_candidates_penalized(A(b["logits"]), V, A(b["scores"]), B, K, V, do_sample, top_k, 1.0, 1.0, 1,
                                             0, 0, NC, hist, ld, n_hist, p, A(b["tok"]), A(b["beam"]), A(b["out"]),
                                             A(b["ws"]), 8192, None)


def test_abi_version_is_still_8():
    from projectiontrainer_amd import _lib as L
    assert L.lib().ptk_abi_version() == 8


@pytest.mark.parametrize("call", [_sample, _beam])
def test_penalty_argument_checks_need_no_gpu(call):
    from projectiontrainer_amd import _lib as L
    lib = L.lib()
    b = _buffers()
    err = lib.ptk_last_error
    for p in (0.0, -1.5, float("nan"), float("inf")):
        assert call(lib, b, A(b["hist"]), 8, 4, p) != 0 and b"repetition_penalty" in err(), p
    assert call(lib, b, None, 8, 4, 1.8) != 0 and b"history is NULL" in err()
    assert call(lib, b, A(b["hist"]), 3, 4, 1.8) != 0 and b"history_ld" in err()
    assert call(lib, b, A(b["hist"]), 8, -1, 1.8) != 0 and b"n_hist" in err()
    # the same three hold with the penalty off: the arguments are checked whatever path would run
    assert call(lib, b, None, 8, 4, 1.0) != 0 and b"history is NULL" in err()
    # capacity: top-k + history above the 1024 entries of the LDS lists (no kernel: host memory untouched)
    assert call(lib, b, A(b["hist"]), 2048, 1025, 1.8) != 0 and b"1024" in err()
    assert call(lib, b, A(b["hist"]), 2048, 1000, 1.8, do_sample=1, top_k=25) != 0 and b"1024" in err()
    assert call(lib, b, A(b["hist"]), 2048, 1000, 1.8, do_sample=1, top_k=0) != 0 and b"1024" in err()   # kk = V
    assert not any(b["tok"]) and not any(b["out"]) and bytes(b["ws"]) == bytes(8192)


@pytest.mark.parametrize("p", [1.0, 1.8])
def test_step_rules_are_checked_before_any_device_call(p):
    """temperature, top_p and the shape limits fail in the entry point itself, penalised or not: ahead of the
    zeroing of the status word and of the stand-in `finished` flags (host memory comes back untouched)."""
    from projectiontrainer_amd import _lib as L
    lib = L.lib()
    b = _buffers()
    err = lib.ptk_last_error
    h = A(b["hist"])

    def sample(temperature, top_p):
        return lib.ptk_sample_next_token(A(b["logits"]), V, B, V, 1, 10, temperature, top_p, 0, 0, -1, 0, None, h, 8, 4,
                                         p, A(b["tok"]), A(b["ws"]), 8192, None)

    def beam(temperature=1.0, top_p=1.0, beams=K, n_cand=NC, ws_bytes=8192):
        return lib.ptk_beam_candidates_penalized(A(b["logits"]), V, A(b["scores"]), B, beams, V, 1, 10, top_p,
                                                 temperature, 1, 0, 0, n_cand, h, 8, 4, p, A(b["tok"]), A(b["beam"]),
                                                 A(b["out"]), A(b["ws"]), ws_bytes, None)
    assert sample(0.0, 1.0) != 0 and b"temperature" in err()
    assert sample(1.0, 1.5) != 0 and b"top_p" in err()
    assert beam(temperature=-1.0) != 0 and b"temperature" in err()
    assert beam(top_p=1.5) != 0 and b"top_p" in err()
    assert beam(beams=9) != 0 and b"beams" in err()
    assert beam(n_cand=33) != 0 and b"n_cand" in err()
    need = (lib.ptk_beam_candidates_penalized_workspace_bytes if p != 1.0 else lib.ptk_beam_candidates_workspace_bytes)
    assert beam(ws_bytes=need(B, K, NC) - 1) != 0 and b"workspace" in err()
    assert not any(b["tok"]) and not any(b["out"]) and bytes(b["ws"]) == bytes(8192)


def test_generate_penalized_argument_checks_need_no_gpu():
    from projectiontrainer_amd import _lib as L
    lib = L.lib()
    cfg = L.Gemma3ConfigC(V, 32, 64, 1, 2, 1, 16, 8, 6, 0, 16.0, 1e-6)
    w = L.Gemma3WeightsC()
    x = (ctypes.c_float * 64)()
    out = (ctypes.c_int64 * 4096)()
    ws = (ctypes.c_char * 64)()

    def run(p, nt=8, do_sample=0, top_k=0):
        d = L.Gemma3GenerateC(1, 4, nt, do_sample, top_k, 1.0, 0, -1, 0, 4, 1.0)
        return lib.ptk_gemma3_generate_penalized(cfg, w, d, A(x), None, A(out), None, p, A(ws), 64, None)
    for p in (0.0, -2.0, float("nan"), float("inf")):
        assert run(p) != 0 and b"repetition_penalty" in lib.ptk_last_error(), p
    # the longest history (max_new_tokens - 1) with the top-k must fit, checked before the prefill
    assert run(1.8, nt=1026) != 0 and b"1024" in lib.ptk_last_error()
    assert run(1.8, nt=1000, do_sample=1, top_k=50) != 0 and b"1024" in lib.ptk_last_error()
    d = L.Gemma3GenerateC(1, 4, 8, 1, 10, 0.0, 0, -1, 0, 4, 1.0)   # temperature 0 with a penalty: before the prefill
    assert lib.ptk_gemma3_generate_penalized(cfg, w, d, A(x), None, A(out), None, 1.8, A(ws), 64, None) != 0
    assert b"temperature" in lib.ptk_last_error()
    assert (lib.ptk_gemma3_generate_penalized_workspace_bytes(cfg, 1, 4, 8)
            > lib.ptk_gemma3_generate_workspace_bytes(cfg, 1, 4, 8))
    assert not any(out)
