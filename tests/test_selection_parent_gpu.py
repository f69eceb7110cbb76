"""The token-selection entry points (ptk_sample_next_token, ptk_beam_candidates, ptk_beam_candidates_penalized)
against a table recorded bit for bit from the parent commit's library on the MI355X
(tests/golden/selection_parent.npz, tools/selection_table.py): return code, tokens, beam indices, score bits and the
finished flags of every case.  The other GPU tests check the selections against HF-style references through
distribution laws and greedy equality; this one pins the draw of a given seed, so a rewrite of the kernels cannot
move it unseen."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("selection_table", os.path.join(ROOT, "tools", "selection_table.py"))
_tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_tool)   # (importing the tool touches neither the environment nor the library)
TABLE = os.path.join(ROOT, "tests", "golden", "selection_parent.npz")
CASES = _tool.cases()


def test_case_list_covers_every_path():
    """No GPU: the list names each path it reaches, and none may go missing; the fixture holds every case."""
    have = set().union(*[c["paths"] for c in CASES])
    assert not (_tool.REQUIRED_PATHS - have), sorted(_tool.REQUIRED_PATHS - have)
    for c in CASES:   # what the names promise
        p = c["paths"]
        if "sample.chunked_draw_no_threshold" in p:
            assert c["do_sample"] and c["top_k"] == 0 and c["top_p"] == 1.0 and c["V"] > 1024
        if "sample.chunked_draw_threshold" in p:
            assert c["do_sample"] and c["top_k"] == 600 and c["top_p"] == 1.0 and c["V"] > 1024
        if "unaligned_rows" in p:
            assert (c["V"] + c["ld_extra"]) * 2 % 16
        if "penalty" in p:
            assert c["penalty"] != 1.0 and c["n_hist"] > 0
    for kind, base in (("sample", "sample.greedy"), ("sample", "sample.k50_p0.9"), ("beam", "beam.greedy"),
                       ("beam", "beam.k50_p0.9_min_keep2")):
        plain = [c for c in CASES if base in c["paths"] and "penalty" not in c["paths"]]
        assert plain
        for c in plain:   # each greedy and each (50, 0.9) case again with p in {1.8, 0.6} x n_hist in {1, 70}
            got = {(d["penalty"], d["n_hist"]) for d in CASES if d["id"].startswith(c["id"] + ".p")}
            assert got == set(_tool.PEN_VARIANTS), c["id"]
    rec = np.load(TABLE)
    keys = set(rec.files)
    for c in CASES:
        want = {"rc", "tok", "finished"} if c["kind"] == "sample" else {"rc", "tok", "beam", "score_bits"}
        assert {f"{c['id']}/{k}" for k in want} <= keys, c["id"]
    # the recorded overflow behaviour: the arg-max fallback, no candidates, and the error return (not a fault)
    assert rec["sample.overflow.V4104/rc"][0] == 0 and rec["sample.overflow.V4104/tok"][0] == 0
    assert rec["beam.overflow.V4104/rc"][0] == 0 and (rec["beam.overflow.V4104/tok"][0] == -1).all()
    assert rec["sample.overflow.pen.V4104/rc"][0] == -1 and rec["beam.overflow.pen.V4104/rc"][0] == -1


@pytest.mark.gpu
def test_selection_matches_parent_table(gpu):
    rec = np.load(TABLE)
    bad = []
    for c in CASES:
        got = _tool.run_case(c, gpu)
        for k, v in got.items():
            want = rec[f"{c['id']}/{k}"]
            if v.dtype != want.dtype or not np.array_equal(v, want):
                bad.append((c["id"], k, v.ravel()[:8].tolist(), want.ravel()[:8].tolist()))
    assert not bad, bad[:10]
