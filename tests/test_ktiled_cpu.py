"""The k-step-tiled weight layout's offset function (gemm_plan.cpp kstep_tile_offset, through
ptk_kstep_tile_offset) against a numpy restatement of the layout's definition.  No GPU."""
import numpy as np
import pytest

from tests.ktiled_util import tiled_source_index


@pytest.mark.parametrize("N", [16, 48, 272])
@pytest.mark.parametrize("K", [32, 64, 1152])
def test_kstep_tile_offset_matches_definition(N, K):
    from projectiontrainer_amd import _lib as L
    f = L.lib().ptk_kstep_tile_offset
    src = tiled_source_index(N, K)                      # tiled element j holds row-major element src[j]
    assert np.array_equal(np.sort(src), np.arange(N * K))   # the definition itself is a permutation
    want = np.empty(N * K, np.int64)                    # row-major element -> byte offset in the tiled copy
    want[src] = 2 * np.arange(N * K)
    got = np.array([f(r, k, K) for r in range(N) for k in range(K)], np.int64)
    assert np.array_equal(got, want)
    # every (row, k) exactly once, within the copy's N * K * 2 bytes
    assert np.array_equal(np.sort(got), 2 * np.arange(N * K))
    # rows past N (the zero-filled rest of the last 256-row column tile) lie at or past the buffer's end
    past = np.array([f(r, k, K) for r in range(N, N + 256) for k in (0, 7, 8, K - 1)], np.int64)
    assert past.min() >= N * K * 2
