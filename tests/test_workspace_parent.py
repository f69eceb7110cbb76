"""The Gemma3 workspace sizes against the parent commit's (tests/golden/selection_parent.npz, recorded by
tools/selection_table.py): ptk_gemma3_workspace_bytes, _train_, _generate_ and _decode_workspace_bytes for the tiny,
cfg2 and cfg5 presets.  The layout functions in models.cpp size and carve the workspace in one pass, so removing a
member or a helper there must not move a byte.  No GPU: the queries launch nothing."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("selection_table", os.path.join(ROOT, "tools", "selection_table.py"))
_tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_tool)


def test_workspace_bytes_match_parent():
    rec = np.load(os.path.join(ROOT, "tests", "golden", "selection_parent.npz"))
    got = _tool.workspace_table()
    assert len(got) == 12 and {k.split("/")[1] for k in got} == {"tiny", "cfg2", "cfg5"}
    assert all(v > 0 for v in got.values())
    assert {k: int(rec[k][0]) for k in got} == got
