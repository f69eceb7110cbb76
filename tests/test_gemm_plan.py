"""The host-side GEMM dispatch planner (csrc/gemm_plan.cpp) against a table recorded from the parent commit's library
(tests/data/gemm_dispatch_parent.json, tools/gemm_dispatch_table.py): the kernel family, the 8-wave kernel's tile rows
and the stream-K split of every GEMM shape the benchmarked steps launch plus the boundary rows of each predicate, and
gemm_split's K split of the Stage-2 / cfg1 shapes.  No GPU: ptk_gemm_plan / ptk_gemm_split_plan launch nothing."""
import ctypes as C
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gemm_dispatch_table", os.path.join(ROOT, "tools", "gemm_dispatch_table.py"))
_tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_tool)
gemm_desc_from_row = _tool.gemm_desc_from_row   # (importing the tool touches neither the environment nor the library)
TABLE = os.path.join(ROOT, "tests", "data", "gemm_dispatch_parent.json")


@pytest.fixture(scope="module")
def table():
    t = json.load(open(TABLE))
    assert t["ncu"] == 256 and 150 <= len(t["rows"]) and len(t["split_rows"]) >= 20
    return t


def test_plan_matches_parent_table(table):
    """(path, tile rows, tail split) of every row.  The table's tail_split_raw is the parent's ptk_gemm_tail_split,
    which plans without launch_gemm's gates: a launch carries that split exactly when its path is p8sk, and
    ptk_gemm_tail_split itself still answers the raw value.  tile_rows is recorded for the p8 rows; every other
    family has 256-row tiles in the plan."""
    from projectiontrainer_amd import _lib as L
    lib = L.lib()
    bad = []
    try:
        for r in table["rows"]:
            L.check(lib.ptk_gemm_force_small_tiles(r.get("force", 0)), "force")
            d = gemm_desc_from_row(r)
            path, tm, split = C.c_int(-1), C.c_int(-1), C.c_int(-1)
            L.check(lib.ptk_gemm_plan(d, table["ncu"], C.byref(path), C.byref(tm), C.byref(split)), "ptk_gemm_plan")
            got = (L.GEMM_PATHS[path.value], tm.value, split.value, lib.ptk_gemm_tail_split(d))
            want = (r["path"], r["tile_rows"] or 256, r["tail_split_raw"] if r["path"] == "p8sk" else 0,
                    r["tail_split_raw"])
            if got != want:
                bad.append((r["label"], got, want))
    finally:
        lib.ptk_gemm_force_small_tiles(0)
    assert not bad, bad
    paths = {r["path"] for r in table["rows"]}
    assert paths >= {"nt128", "nt128b", "big", "big2", "w4", "p8", "p8sk"}
    assert {r["tile_rows"] for r in table["rows"] if r["path"] == "p8"} == {256, 224, 192, 160}


def test_split_plan_matches_parent_table(table):
    """gemm_split's decision (slices, kc, remainder, split-K scratch lent to the stream-K tail) for the shapes
    gemma_run routes through it: Stage 2's M 14 336 / 7 168 projections and transpose-path weight grads, cfg1's
    M 640 shapes, the Stage-1 steps' (which stay unsplit), and K splits with an odd K-tile count (one full slice
    plus a remainder slice: slices == 1 with kc != 0).  kc == 0 means one unsplit launch, and only then."""
    from projectiontrainer_amd import _lib as L
    lib = L.lib()
    bad = []
    for r in table["split_rows"]:
        d = gemm_desc_from_row(r)
        out = [C.c_int(-1) for _ in range(4)]
        L.check(lib.ptk_gemm_split_plan(d, table["ncu"], r["part_floats"], *[C.byref(o) for o in out]), "split_plan")
        got = tuple(o.value for o in out)
        want = (r["slices"], r["kc"], r["rem"], r["tail_ws"])
        if got != want:
            bad.append((r["label"], got, want))
        kc, K = got[1], r["K"]
        if kc == 0:   # unsplit: nothing else set but the lent scratch
            assert got[0] == 1 and got[2] == 0, (r["label"], got)
        else:         # the slices cover K exactly, none lends the scratch
            assert got[0] >= 1 and got[0] * kc + got[2] == K and 0 <= got[2] < kc and not got[3], (r["label"], got)
    assert not bad, bad
    assert any(r["slices"] > 1 and r["rem"] for r in table["split_rows"])
    assert any(r["slices"] == 1 and r["kc"] and r["rem"] for r in table["split_rows"])   # odd K-tile count
    assert any(r["tail_ws"] for r in table["split_rows"])
