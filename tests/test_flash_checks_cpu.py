"""Self-test of tests/flash_util.py (CPU): for every input family of tests/test_flash_exact_gpu.py the emulation of
the kernels passes every checker at half the bar, the inputs meet their preconditions (bounded scores for the
readouts, rescale events for the dynamic-range rows), and every fault the GPU tests are meant to see is rejected
when it is injected into the emulation or the reference."""
import functools
import math

import pytest
import torch

from tests import flash_util as U

FAMILIES = ("F1", "F2", "F3", "F4", "F5", "F6", "F7")


@functools.lru_cache(maxsize=None)
def _cases(fam):
    return tuple(c for f, c in U.all_cases() if f == fam)


@functools.lru_cache(maxsize=None)
def _ref(fam, i):
    """(case, mask, float64 reference, emulation) of case i of a family; computed once, never modified."""
    c = _cases(fam)[i]
    return c, U.case_mask(c), U.ref_of(c), U.emu_of(c)


def _pick(fam, **want):
    for i, c in enumerate(_cases(fam)):
        if all(getattr(c, k) == v for k, v in want.items()):
            return _ref(fam, i)
    raise KeyError(want)


def _rejected(fam, c, ref, got, m, **kw):
    with pytest.raises(AssertionError):
        U.check_family(fam, c, ref, got, m, **kw)


@pytest.mark.parametrize("fam", FAMILIES)
def test_emulation_within_half_bar(fam):
    """The kernels' rounding points alone stay within half of every bar on every case, and the measured worst
    ratios do not exceed the E_* the bars are derived from."""
    for i in range(len(_cases(fam))):
        c, m, ref, emu = _ref(fam, i)
        got = U.check_family(fam, c, ref, emu, m, frac=0.5)
        for k, v in got.items():
            what, _, kind = k.partition(" ")
            if what != "LSE":
                assert v <= (U.E_ROWS if what == "rows" else U.E_READ)[kind], (c.name, k, v)


@pytest.mark.parametrize("fam", ("F1", "F2", "F3", "F5"))
def test_readout_scores_bounded(fam):
    """No P of a live row, over the visible keys and over every key a wrong mask could admit (the cache's bait rows
    included), is below 1e-30: a leak cannot underflow to the exact zero the test expects, and no expected entry is
    lost to the floor."""
    for i in range(len(_cases(fam))):
        c, m, ref, _ = _ref(fam, i)
        K = c.Kcache if hasattr(c, "Kcache") else c.K
        s = (c.Q.double() @ K.double().transpose(-1, -2)) * c.scale
        live = torch.isfinite(ref.LSE)
        p = torch.exp(s - ref.LSE.masked_fill(~live, 0.0)[..., None])[live]
        assert float(p.min()) >= U.P_MIN, (c.name, float(p.min()))


def test_dynamic_range_event_counts():
    """F4 preconditions from the float64 scores.  Non-causal cases: at least 3/4 of the rows rescale after their first
    tile (the fourth pattern, monotone decreasing, never does).  Causal cases: the same among the rows that see
    three tiles or more (a row inside its first tile has nothing to rescale, and the 7.9 + 0.3 pattern fires on its
    third).  Some row rescales >= 6 times at 32-key tiles (hd 256) and at 64-key tiles (hd 64; that needs more
    than the 5 tiles of 320 keys: the 512-key case)."""
    most = {}
    for i, c in enumerate(_cases("F4")):
        c, m, ref, emu = _ref("F4", i)
        ev = U.rescale_events(c.Q.double() @ c.K.double().transpose(-1, -2), m, c.tile, c.scale)
        assert torch.equal(ev, emu.events)
        ntiles = (m.reshape(c.Z, c.rows, -1, c.tile).any(-1)).sum(-1)
        rows = ntiles >= 3 if c.causal else torch.ones_like(ntiles, dtype=torch.bool)
        if c.D == 256 or not c.causal:      # (hd 64 causal: 64 rows, all inside the first 64-key tile)
            assert float(rows.double().mean()) >= 0.75
            assert float((ev[rows] >= 1).double().mean()) >= 0.75, c.name
        most[c.tile] = max(most.get(c.tile, 0), int(ev.max()))
    assert most[32] >= 6 and most[64] >= 6, most


def test_existing_inputs_have_no_events():
    """What the issue measured: N(0, 1) operands at scale D^-0.5 (the older kernel tests) rescale on next to no row."""
    g = torch.Generator().manual_seed(0)
    q, k = (torch.randn(1280, 256, generator=g).bfloat16().double() for _ in range(2))
    ev = U.rescale_events(q[None] @ k[:320].T[None], U.mask(1280, 320, qdiv=4, causal=True), 32, 256 ** -0.5)
    assert int((ev > 0).sum()) <= 4


# ---------------------------------------------------------------------------------------- mutated masks
def _emu_masked(c, m):
    return U.emu_of(c, m=m)


@pytest.mark.parametrize("window,dw", [(w, d) for w in (1, 2, 32, 33, 64, 255, 256) for d in (-1, 1) if w + d > 0])
def test_window_off_by_one_rejected(window, dw):
    c, m, ref, _ = _pick("F1", window=window, rows=1280)
    _rejected("F1", c, ref, _emu_masked(c, U.case_mask(c, window=window + dw)), m)


@pytest.mark.parametrize("fam,want", (("F1", dict(window=33, rows=1280)), ("F1", dict(window=0, rows=1280)),
                                      ("F2", dict(window=63))))
@pytest.mark.parametrize("dd", (-1, 1))
def test_causal_diagonal_off_by_one_rejected(fam, want, dd):
    c, m, ref, _ = _pick(fam, **want)
    _rejected(fam, c, ref, _emu_masked(c, U.case_mask(c, diag=dd)), m)


@pytest.mark.parametrize("fam,want,b,key", (("F1", dict(window=0, rows=1280), 1, 207), ("F1", dict(window=100, rows=1280), 0, 69),
                                            ("F2", dict(window=64), 0, 3), ("F3", dict(nkeys=332, G=4), 1, 167)))
def test_ignored_key_valid_flag_rejected(fam, want, b, key):
    c, m, ref, _ = _pick(fam, **want)
    kv = c.key_valid.clone()
    assert kv[b, key] == 0
    kv[b, key] = 1
    _rejected(fam, c, ref, _emu_masked(c, U.case_mask(c, key_valid=kv)), m)


@pytest.mark.parametrize("G,nkeys", ((1, 5), (4, 32), (8, 333)))
def test_key_past_nkeys_rejected(G, nkeys):
    """A decode launch that reads one cache row past nkeys picks up the bait."""
    c, m, ref, _ = _pick("F3", G=G, nkeys=nkeys, key_valid=None)
    lo, hi = c.offset, c.offset + nkeys + 1
    more = U.emulate(c.Q, c.Kcache[:, lo:hi], c.Vcache[:, lo:hi], None, torch.ones(c.Z, c.rows, nkeys + 1, dtype=torch.bool),
                     c.scale, tile=c.tile)
    _rejected("F3", c, ref, more, m)


@pytest.mark.parametrize("fam,want,tile", (("F1", dict(window=0, rows=1280), 4), ("F1", dict(window=100, rows=1280), 7),
                                           ("F2", dict(window=64), 1), ("F7", dict(window=512, nkeys=704), 9)))
def test_dropped_key_tile_rejected(fam, want, tile):
    c, m, ref, _ = _pick(fam, **want)
    mm = m.clone()
    mm[:, :, 32 * tile:32 * tile + 32] = False
    _rejected(fam, c, ref, _emu_masked(c, mm), m)


@pytest.mark.parametrize("fam,want,drop", (("F5", dict(rows=256, G=1, window=0, kind="qI"), (1, 96, 128, 0, 128)),
                                           ("F5", dict(rows=256, G=4, window=33, kind="qI"), (0, 128, 160, 0, 64)),
                                           ("F6", dict(window=0), (37, 192, 224, 0, 64))))
def test_dropped_row_chunk_of_a_key_slab_rejected(fam, want, drop):
    """dK / dV of one 128-key slab miss one 32-row chunk of queries."""
    c, m, ref, emu = _pick(fam, **want)
    bad = U.ref_of(c, drop=drop)
    for k in ("dK", "dV"):
        got = type(emu)(**{k: U.bf16r(getattr(bad, k))})
        _rejected(fam, c, ref, got, m)


def test_skipped_alpha_rejected():
    """One row's O misses one rescale (its row sum does not): the dynamic-range rows see it."""
    seen = 0
    for i, c in enumerate(_cases("F4")):
        c, m, ref, emu = _ref("F4", i)
        if int(emu.events.max()) == 0:      # hd 64 causal: 64 rows inside one 64-key tile
            continue
        seen += 1
        z, row = (emu.events == emu.events.max()).nonzero()[0].tolist()
        # the staircase row's last rescale and a spike row's only one (an early step of a staircase is invisible:
        # what it fails to scale down ends 9 log2 units per later tile below the output's last bit)
        spike = [(zz, r) for zz in range(c.Z) for r in range(c.rows - 1, 0, -1) if (r + zz) % 4 == 3 and emu.events[zz, r] == 1][0]
        for z, row, n in ((z, row, int(emu.events.max()) - 1), (*spike, 0)):
            bad = U.emu_of(c, skip_alpha=(z, row, n))
            assert not torch.equal(bad.O, emu.O)
            _rejected("F4", c, ref, type(emu)(O=bad.O), m)
    assert seen >= 4


@pytest.mark.parametrize("fam", FAMILIES)
def test_shifted_lse_rejected(fam):
    c, m, ref, emu = _ref(fam, 0)
    for sign in (-1, 1):
        live = torch.isfinite(ref.LSE)
        lse = torch.where(live, emu.LSE + sign * math.log(1 + 1 / 512), emu.LSE)
        _rejected(fam, c, ref, type(emu)(LSE=lse), m)


@pytest.mark.parametrize("window", U.F6_WINDOWS)
def test_output_in_the_neighbouring_z_rejected(window):
    c, m, ref, emu = _pick("F6", window=window)
    for k in ("O", "dQ", "dK", "dV"):
        x = getattr(emu, k).clone()
        x[[40, 41]] = x[[41, 40]]
        _rejected("F6", c, ref, type(emu)(**{k: x}), m)
    lse = emu.LSE.clone()
    lse[[40, 41]] = lse[[41, 40]]
    _rejected("F6", c, ref, type(emu)(LSE=lse), m)


def test_mask_restates_flash_args():
    """mask() against a key-by-key statement of the rule."""
    kv = torch.ones(2, 12, dtype=torch.int32)
    kv[1, 2] = 0
    m = U.mask(9, 12, qdiv=3, causal=True, window=2, key_valid=kv)
    for b in range(2):
        for r in range(9):
            for k in range(12):
                q = r // 3
                assert bool(m[b, r, k]) == (k <= q and k > q - 2 and bool(kv[b, k]))
    m = U.mask(4, 12, window=2, key_len=7)          # a window without causal is no window
    assert m.shape == (1, 4, 12) and bool(m[0, :, :7].all()) and not bool(m[0, :, 7:].any())
