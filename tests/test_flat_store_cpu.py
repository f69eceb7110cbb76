"""FlatStore's layout and upkeep on the CPU (no GPU, no libptk): saved optimizer shards depend on the offsets, the
padding and `numel`, so they are written out literally here."""
import torch

from projectiontrainer_amd.flat_store import FlatStore

SEGS = [("a", (3, 5)), ("b", (7,)), ("c", (2, 64))]
MIRRORED = [("m", (5,)), ("n", (64,))]


def build(**kw):
    return FlatStore(SEGS, MIRRORED, device="cpu", align=64, pad_to=192, **kw)


def test_layout_is_the_recorded_one():
    st = build()
    assert st.offsets == {"a": (0, (3, 5)), "b": (64, (7,)), "c": (128, (2, 64)), "m": (256, (5,)), "n": (320, (64,))}
    assert (st.mirror_lo, st.mirror_hi) == (256, 384)
    assert st.numel == 384
    assert st.flat.shape == st.grad.shape == (384,) and st.flat.dtype == st.grad.dtype == torch.bfloat16
    assert st.mirror.shape == (128,) and st.mirror.dtype == torch.float32
    assert not hasattr(st, "exp_avg") and not hasattr(st, "sumsq")


def test_pad_to_rounds_numel_up_and_its_absence_does_not():
    assert FlatStore(SEGS[:2], device="cpu").numel == 128
    assert FlatStore(SEGS[:2], device="cpu", pad_to=192).numel == 192
    assert FlatStore(SEGS, MIRRORED, device="cpu", pad_to=256).numel == 512
    st = FlatStore(SEGS[:2], device="cpu")
    assert (st.mirror_lo, st.mirror_hi) == (128, 128) and not hasattr(st, "mirror")


def test_moments_on_request():
    st = build(moments=True)
    for buf in (st.exp_avg, st.exp_avg_sq):
        assert buf.shape == (384,) and buf.dtype == torch.bfloat16 and not buf.any()
    assert st.sumsq.shape == (1,) and st.sumsq.dtype == torch.float32
    assert len({t.data_ptr() for t in (st.flat, st.grad, st.exp_avg, st.exp_avg_sq)}) == 4


def test_views_alias_the_buffers_and_gaps_stay_zero():
    st = build(moments=True)
    for k, (name, shape) in enumerate(SEGS + MIRRORED):
        v, g, m = st.view(name), st.grad_view(name), st.view(name, st.exp_avg)
        assert v.shape == g.shape == m.shape == shape
        off = st.offsets[name][0]
        for t, buf in ((v, st.flat), (g, st.grad), (m, st.exp_avg)):
            assert t.data_ptr() == buf.data_ptr() + 2 * off
        v.fill_(k + 1)
        g.fill_(-(k + 1))
    want = torch.zeros(384)
    for k, (off, n) in enumerate(((0, 15), (64, 7), (128, 128), (256, 5), (320, 64))):
        want[off:off + n] = k + 1
    assert torch.equal(st.flat.float(), want)          # every element outside a segment is still zero
    assert torch.equal(st.grad.float(), -want)
    assert not st.exp_avg.any() and not st.exp_avg_sq.any()


def test_mirror_follows_the_store_on_refresh_only():
    st = build()
    g = torch.Generator().manual_seed(0)
    st.flat.copy_(torch.randn(384, generator=g))
    assert not st.mirror.any()
    st.refresh_mirror()
    for name, shape in MIRRORED:
        m = st.mirror_view(name)
        assert m.shape == shape and m.dtype == torch.float32
        assert m.data_ptr() == st.mirror.data_ptr() + 4 * (st.offsets[name][0] - 256)
        assert torch.equal(m, st.view(name).float())
    assert torch.equal(st.mirror, st.flat[256:384].float())
    before = st.mirror.clone()
    st.view("m").zero_()
    assert torch.equal(st.mirror, before)


def test_zero_grad_clears_the_grads_only():
    st = build(moments=True)
    for buf in (st.flat, st.grad, st.exp_avg, st.exp_avg_sq):
        buf.fill_(1)
    st.refresh_mirror()
    st.zero_grad()
    assert not st.grad.any()
    assert all(bool((buf == 1).all()) for buf in (st.flat, st.exp_avg, st.exp_avg_sq, st.mirror))
