"""The kernels that turn gradients into new weights, each against a plain reference of the same operation.

ptk_bf16_grad_scale_sumsq   vs a float64 sum of squares and a one-multiply-one-rounding transcription
ptk_adamw_bf16              vs torch.optim.AdamW(foreach=False) + clip_grad_norm_(foreach=False) on CPU bf16
                            tensors (the kernel documents itself as exactly that, every op rounded to bf16)
ptk_clip_adamw (fp32)       vs the same torch pair on float64 copies, with torch's own float32 run as the yardstick

The end-to-end goldens accept parameters within 2.5 * sum(lr) of the reference after AdamW, which is the size of
a whole Adam step: a wrong bias correction, a dropped rounding or a wrong clip coefficient passes them.  These
tests work at one bf16 / fp32 ulp, and reach the second grid-stride pass, the vector bodies' tails and the three
clip states that the tiny and cfg4-width presets never do."""
import math

import numpy as np
import pytest
import torch

from tests.test_stage2_gpu import record   # the suite's one parity-metrics log

pytestmark = pytest.mark.gpu


def f32(x):
    """The value a C float argument carries."""
    return float(np.float32(x))


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def bf16_of(x):
    """A Python float rounded to bf16 (through float32, as the kernel's sqrtf result is)."""
    return float(torch.tensor(x, dtype=torch.float32).bfloat16())


# ---------------------------------------------------------------- the kernels under test
def scale_sumsq(g, scale, out=None):
    """ptk_bf16_grad_scale_sumsq on the device tensor g (in place); returns the device [1] fp32 sum."""
    from projectiontrainer_amd import _lib as L
    partial = torch.empty(L.lib().ptk_bf16_sumsq_partial_floats(), dtype=torch.float32, device=g.device)
    if out is None:
        out = torch.full((1,), 123.0, dtype=torch.float32, device=g.device)
    L.check(L.lib().ptk_bf16_grad_scale_sumsq(g.data_ptr(), g.numel(), scale, partial.data_ptr(), out.data_ptr(),
                                              L.stream_ptr(g.device)), "ptk_bf16_grad_scale_sumsq")
    return out


def adamw_bf16(p, g, m, v, sumsq, max_norm, lr, step, norm_out, hp):
    from projectiontrainer_amd import _lib as L
    return L.lib().ptk_adamw_bf16(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(),
                                  sumsq.data_ptr(), max_norm, lr, hp["betas"][0], hp["betas"][1], hp["eps"],
                                  hp["weight_decay"], step, norm_out.data_ptr(), L.stream_ptr(p.device))


def clip_adamw(p, g, m, v, grad_scale, max_norm, lr, step, norm_out, hp):
    from projectiontrainer_amd import _lib as L
    partial = torch.empty(1024, dtype=torch.float32, device=p.device)
    return L.lib().ptk_clip_adamw(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), grad_scale,
                                  max_norm, lr, hp["betas"][0], hp["betas"][1], hp["eps"], hp["weight_decay"], step,
                                  partial.data_ptr(), norm_out.data_ptr(), L.stream_ptr(p.device))


# ---------------------------------------------------------------- ptk_bf16_grad_scale_sumsq
# 0; 1 and 7: only the scalar tail; 8: one vector, no tail; 9 and 2051: vectors + tail;
# 2 * 1024 * 2048 + 5: every thread's second grid-stride pass, and a tail after it
SUMSQ_SIZES = [0, 1, 7, 8, 9, 2051, 2 * 1024 * 2048 + 5]


@pytest.mark.parametrize("scale", [1.0, 0.5, 1.0 / 3.0], ids=["s1", "s0.5", "s1_3"])
@pytest.mark.parametrize("n", SUMSQ_SIZES)
def test_bf16_grad_scale_sumsq(gpu, n, scale):
    """out vs a float64 sum of squares of the scaled-and-rounded grads within 1e-5 relative: at the largest n a
    value passes fewer than 40 fp32 roundings (two 8-wide adds per thread, an 8-level block tree, 4 partials per
    thread, a second tree), under 2.4e-6 worst case.  g = bf16(g * scale) to the bit (one multiply and one
    rounding: nothing to contract), untouched for scale 1; two calls on equal input give bit-equal sums."""
    gen = torch.Generator().manual_seed(1000 + n % 997)
    g0 = torch.randn(n, generator=gen).mul_(0.37).bfloat16()
    want_g = g0 if scale == 1.0 else (g0.float() * torch.tensor(scale, dtype=torch.float32)).bfloat16()
    want = float((want_g.double() ** 2).sum())
    g = g0.to(gpu, copy=True)
    out = scale_sumsq(g, scale)
    g2 = g0.to(gpu, copy=True)
    out2 = scale_sumsq(g2, scale)
    torch.cuda.synchronize()
    got = float(out)
    rel = abs(got - want) / want if want else abs(got)
    print(f"scale_sumsq n={n} scale={scale:.6g}: got {got!r} want {want!r} rel {rel:.3e}")
    record("bf16_grad_scale_sumsq", f"n{n}_s{scale:.4g}", rel_err=rel)
    if n == 0:
        assert got == 0.0
    assert rel <= 1e-5, (got, want)
    assert torch.equal(bits(g), bits(want_g)), "g is not bf16(g * scale) to the bit"
    assert torch.equal(out2.cpu().view(torch.int32), out.cpu().view(torch.int32)), "two calls on equal input differ"
    assert torch.equal(bits(g2), bits(g))


def test_bf16_grad_scale_sumsq_rejects_misaligned(gpu):
    """g is loaded 16 bytes at a time: a shard offset that is no multiple of 8 elements is an error before any
    launch, and neither g nor out is touched."""
    from projectiontrainer_amd import _lib as L
    buf = torch.randn(64).bfloat16().to(gpu, copy=True)
    keep = bits(buf)
    partial = torch.empty(L.lib().ptk_bf16_sumsq_partial_floats(), dtype=torch.float32, device=gpu)
    out = torch.full((1,), 123.0, dtype=torch.float32, device=gpu)
    for off in (1, 3, 7):
        rc = L.lib().ptk_bf16_grad_scale_sumsq(buf[off:].data_ptr(), 40, 0.5, partial.data_ptr(), out.data_ptr(),
                                               L.stream_ptr(gpu))
        assert rc != 0 and b"16-byte aligned" in L.lib().ptk_last_error()
    torch.cuda.synchronize()
    assert torch.equal(bits(buf), keep) and float(out) == 123.0
    assert float(scale_sumsq(buf[8:], 1.0)) > 0.0   # 16 bytes in: accepted


# ---------------------------------------------------------------- ptk_adamw_bf16 vs torch on CPU bf16
HP = dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
LRS = [1e-3, 7e-4, 3e-4, 1.3e-3, 5e-5]
# (name, max_norm, the five steps' ||g|| as a multiple of max_norm (of 1 when the clip is off)).  0.3 is no power
# of two: torch's `max_norm / tensor` is reciprocal() * max_norm, two bf16 roundings, which max_norm 1 cannot show
CLIPS = [("off", 0.0, (0.5, 2.0, 8.0, 0.1, 3.0)),
         ("inactive", 1.0, (0.3, 0.7, 0.5, 0.85, 0.2)),
         ("active", 1.0, (1.5, 4.0, 40.0, 1.2, 10.0)),
         ("active0.3", 0.3, (1.5, 4.0, 40.0, 1.2, 10.0))]
# 1; 255 / 257: one block short of and past full; 100 003: many blocks, odd; 4096 * 256 + 77: a second
# grid-stride pass for the first 77 threads
ADAMW_SIZES = [1, 255, 257, 100_003, 4096 * 256 + 77]
ZERO_STEP = 3   # this step's grad has every 7th element zero


def make_grad(n, target_norm, max_norm, seed, zero7):
    """A bf16 grad of about the wanted norm whose bf16 total norm cannot fall on a rounding boundary:
    bf16(sqrt(S (1 +- 4e-4))) is one value for the float64 sum of squares S, and the clip state is the wanted one
    with 10 % to spare.  The kernel's fp32 sum is within 1e-5 of S (test_bf16_grad_scale_sumsq); the margin is
    torch's: its CPU vector_norm accumulates a million fp32 squares to 3.4e-5 of the norm, 7e-5 of S."""
    for k in range(64):
        gen = torch.Generator().manual_seed(seed + k)
        g = torch.randn(n, generator=gen).mul_(target_norm / math.sqrt(n)).bfloat16()
        if zero7:
            g[::7] = 0
            if n == 1:
                return g
        S = float((g.double() ** 2).sum())
        lo, hi = bf16_of(math.sqrt(S * (1 - 4e-4))), bf16_of(math.sqrt(S * (1 + 4e-4)))
        if lo != hi or S == 0.0:
            continue
        if max_norm > 0 and target_norm < max_norm and not lo <= 0.9 * max_norm:
            continue
        if max_norm > 0 and target_norm > max_norm and not lo >= 1.1 * max_norm:
            continue
        return g
    raise AssertionError("no seed with a stable bf16 norm")


def bf16_ulp(x):
    """One bf16 ulp at |x| (float64; 0 at 0): 8 significand bits."""
    x = x.detach().float().abs()
    _, e = torch.frexp(x)
    u = torch.ldexp(torch.ones_like(x, dtype=torch.float64), e - 8)
    return torch.where(x == 0, torch.zeros_like(u), u)


def torch_step(p, opt, g, max_norm, lr):
    """One reference step; returns (norm or None, clipped grad)."""
    opt.param_groups[0]["lr"] = lr
    p.grad = g.clone()
    norm = None
    if max_norm > 0:
        norm = torch.nn.utils.clip_grad_norm_([p], max_norm, foreach=False)
    opt.step()
    return norm, p.grad


def moments(opt, p):
    st = opt.state.get(p, {})
    if "exp_avg" not in st:
        return torch.zeros_like(p.data), torch.zeros_like(p.data)
    return st["exp_avg"].clone(), st["exp_avg_sq"].clone()


@pytest.mark.parametrize("clip", CLIPS, ids=[c[0] for c in CLIPS])
@pytest.mark.parametrize("n", ADAMW_SIZES)
def test_adamw_bf16_vs_torch(gpu, n, clip):
    """Five steps with a changing lr; at every step the kernel starts from torch's p, exp_avg and exp_avg_sq (so
    differences do not compound) and is fed sumsq from ptk_bf16_grad_scale_sumsq.  The total norm and the clipped
    g are torch's to the bit, g is not rewritten unless the clip is active, every element of p, m and v is within
    one bf16 ulp (at the update's largest operand) of torch's, step 1 from zero moments is bit-identical, and at
    n >= 100 003 at most 0.5 % of a tensor's elements differ at all (torch's CPU lerp / addcmul fuse differently
    from a float32 transcription of the kernel in at most 0.06 %; a missing rounding or a wrong constant moves
    whole tensors).  Measured on an MI355X: no element of p, m, v or g differs at any size, clip state or step."""
    name, max_norm, norms = clip
    ci = [c[0] for c in CLIPS].index(name)
    gen = torch.Generator().manual_seed(77 + n)
    p = torch.nn.Parameter(torch.randn(n, generator=gen).mul_(0.05).bfloat16())
    assert bool((p.data != 0).all())
    opt = torch.optim.AdamW([p], lr=LRS[0], foreach=False, **HP)
    b2 = HP["betas"][1]
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for step in range(1, 6):
        lr = LRS[step - 1]
        g0 = make_grad(n, norms[step - 1] * (max_norm if max_norm > 0 else 1.0), max_norm,
                       100_000 * ci + 1000 * step + n % 991, step == ZERO_STEP)
        p_old = p.data.clone()
        m_old, v_old = moments(opt, p)
        if step == 1:
            assert not m_old.any() and not v_old.any()
        # the kernel, from torch's state
        dp, dg, dm, dv = p_old.to(gpu, copy=True), g0.to(gpu, copy=True), m_old.to(gpu, copy=True), v_old.to(gpu, copy=True)
        sumsq = scale_sumsq(dg, 1.0)
        norm_out = torch.full((1,), -7.0, dtype=torch.float32, device=gpu)
        rc = adamw_bf16(dp, dg, dm, dv, sumsq, max_norm, lr, step, norm_out, HP)
        assert rc == 0
        torch.cuda.synchronize()
        # torch
        norm, g_ref = torch_step(p, opt, g0, max_norm, lr)
        m_ref, v_ref = moments(opt, p)
        tag = f"n={n} {name} step {step}"
        if max_norm > 0:
            assert float(norm_out) == float(norm), (tag, float(norm_out), float(norm))
        else:
            assert float(norm_out) == -7.0, f"{tag}: norm_out written with the clip off"
        assert torch.equal(bits(dg), bits(g_ref)), f"{tag}: g is not torch's clipped grad to the bit"
        if name.startswith("active") and bool(g0.any()):   # (n = 1 at the zero step: nothing to clip)
            assert not torch.equal(bits(g_ref), bits(g0)), f"{tag}: the clip was meant to be active"
        else:
            assert torch.equal(bits(dg), bits(g0)), f"{tag}: g rewritten with the clip off / inactive"
        gf = g_ref.float()
        operands = {"p": p_old.float().abs(),
                    "m": torch.maximum(m_old.float().abs(), gf.abs()),
                    "v": torch.maximum(v_old.float().abs(), (1 - b2) * gf.double().pow(2).float())}
        for key, got, ref in (("p", dp, p.data), ("m", dm, m_ref), ("v", dv, v_ref)):
            got = got.cpu()
            d = (got.double() - ref.double()).abs()
            ulp = bf16_ulp(operands[key])
            over = d > ulp
            share = float((got.float() != ref.float()).double().mean())
            worst[key] = max(worst[key], share)
            print(f"adamw_bf16 {tag} {key}: {int((d > 0).sum())} of {n} differ (share {share:.3e}), "
                  f"{int(over.sum())} by more than one ulp, max |d|/ulp "
                  f"{float((d / ulp.clamp_min(1e-300)).max()):.3g}")
            assert not over.any(), f"{tag}: {key} off by more than one bf16 ulp in {int(over.sum())} elements"
            if step == 1:
                assert torch.equal(bits(got), bits(ref)), f"{tag}: {key} not bit-identical at step 1"
            if n >= 100_003:
                assert share <= 5e-3, f"{tag}: {key} differs in {share:.3%} of its elements"
    record("adamw_bf16_vs_torch", f"n{n}_{name}", share_p=worst["p"], share_m=worst["m"], share_v=worst["v"])


def test_adamw_bf16_shards_match_whole_buffer(gpu):
    """The ZeRO-1 property stage2.py relies on: the kernel on [0, h) and [h, n) with the summed sumsq gives p, g,
    m and v bit-identical to one call on the whole buffer.  h is the multiple of 64 nearest n / 2, as the engine's
    shard boundaries are (the sum of squares reads 16 bytes at a time); the clip is active, the moments non-zero."""
    n, h, max_norm, lr, step = 100_003, 50_048, 1.0, 7e-4, 3
    gen = torch.Generator().manual_seed(5)
    p0 = torch.randn(n, generator=gen).mul_(0.05).bfloat16()
    m0 = torch.randn(n, generator=gen).mul_(0.01).bfloat16()
    v0 = torch.randn(n, generator=gen).mul_(0.01).pow_(2).bfloat16()
    g0 = make_grad(n, 4.0, max_norm, 4242, False)

    def fresh():
        return [t.to(gpu, copy=True) for t in (p0, g0, m0, v0)]
    whole = fresh()
    nw = torch.zeros(1, dtype=torch.float32, device=gpu)
    assert adamw_bf16(*whole, scale_sumsq(whole[1], 1.0), max_norm, lr, step, nw, HP) == 0
    parts = fresh()
    lo, hi = [t[:h] for t in parts], [t[h:] for t in parts]
    total = scale_sumsq(lo[1], 1.0) + scale_sumsq(hi[1], 1.0)   # the all-reduce
    ns = torch.zeros(1, dtype=torch.float32, device=gpu)
    assert adamw_bf16(*lo, total, max_norm, lr, step, ns, HP) == 0
    assert adamw_bf16(*hi, total, max_norm, lr, step, ns, HP) == 0
    torch.cuda.synchronize()
    assert float(ns) == float(nw) > 1.1 * max_norm
    assert not torch.equal(bits(whole[1]), bits(g0))
    for key, a, b in zip("pgmv", whole, parts):
        assert torch.equal(bits(a), bits(b)), f"{key}: shards differ from the whole buffer"


def test_adamw_bf16_rejects_step_0(gpu):
    """step counts from 1 (the bias corrections divide by 1 - beta^step): step 0 is an error with a message, and
    nothing is changed."""
    from projectiontrainer_amd import _lib as L
    gen = torch.Generator().manual_seed(9)
    host = [torch.randn(300, generator=gen).mul_(0.05).bfloat16() for _ in range(3)]
    host.append(host[2].float().pow(2).bfloat16())
    dev = [t.to(gpu, copy=True) for t in host]
    sumsq = scale_sumsq(dev[1], 1.0)
    norm_out = torch.full((1,), -7.0, dtype=torch.float32, device=gpu)
    rc = adamw_bf16(*dev, sumsq, 1.0, 1e-3, 0, norm_out, HP)
    assert rc != 0 and b"step" in L.lib().ptk_last_error()
    torch.cuda.synchronize()
    assert float(norm_out) == -7.0
    for a, b in zip(dev, host):
        assert torch.equal(bits(a), bits(b))


# ---------------------------------------------------------------- ptk_clip_adamw (fp32) vs float64
# the hyper-parameters cross the C ABI as floats: every reference gets the values those floats carry
HP32 = dict(betas=(f32(0.9), f32(0.999)), eps=f32(1e-8), weight_decay=f32(0.01))
LRS32 = [f32(1e-3), f32(6e-4), f32(1.2e-3), f32(2e-4)]
# 1 and 3: only the float4 tail; 1027: float4 body + tail; 2 * 1024 * 256 + 3: the norm's and the update's
# second grid-stride pass, and a tail
CLIP32_SIZES = [1, 3, 1027, 2 * 1024 * 256 + 3]


def set_state(opt, p, pv, mv, vv):
    p.data.copy_(pv)
    st = opt.state[p]
    st["exp_avg"].copy_(mv)
    st["exp_avg_sq"].copy_(vv)


@pytest.mark.parametrize("active", [False, True], ids=["inactive", "active"])
@pytest.mark.parametrize("grad_scale", [1.0, 0.125], ids=["gs1", "gs0.125"])
@pytest.mark.parametrize("n", CLIP32_SIZES)
def test_clip_adamw_fp32_vs_float64(gpu, n, grad_scale, active):
    """Four steps against torch.optim.AdamW + clip_grad_norm_(5) on float64 copies, the grads pre-multiplied by
    grad_scale.  Every step starts all three runs (float64, torch's float32 on the CPU, the kernel) from the
    float32 run's state, so nothing compounds.  The bar per tensor (p, m, v, norm) is 4 x the max-abs distance of
    torch's own float32 run from the float64 one on the same inputs (the 4 x for a different summation order of
    the norm and FMA contraction in the update), and at least one fp32 ulp of the tensor's largest magnitude.
    The hyper-parameters reach the kernel as C floats, so all three runs get the values those floats carry.
    Measured on an MI355X, worst kernel distance / bar: p 0.42, m 0.40, v 0.73, norm 0.72."""
    max_norm = 5.0
    gen = torch.Generator().manual_seed(31 + n)
    p32 = torch.nn.Parameter(torch.randn(n, generator=gen).mul_(0.05))
    p64 = torch.nn.Parameter(p32.data.double())
    o32 = torch.optim.AdamW([p32], lr=LRS32[0], foreach=False, **HP32)
    o64 = torch.optim.AdamW([p64], lr=LRS32[0], foreach=False, **HP32)
    worst = {}
    for step in range(1, 5):
        lr = LRS32[step - 1]
        want = (50.0 if active else 2.0) * (0.5 + 0.25 * step)          # ||g * grad_scale||
        g = torch.randn(n, generator=gen).mul_(want / grad_scale / math.sqrt(n))
        if n <= 3:   # a handful of draws: put the norm where the case wants it
            g.mul_(want / grad_scale / float(g.double().norm()))
        p_old = p32.data.clone()
        m_old, v_old = moments(o32, p32)
        dp, dg, dm, dv = p_old.to(gpu, copy=True), g.to(gpu, copy=True), m_old.to(gpu, copy=True), v_old.to(gpu, copy=True)
        norm_out = torch.full((1,), -7.0, dtype=torch.float32, device=gpu)
        rc = clip_adamw(dp, dg, dm, dv, grad_scale, max_norm, lr, step, norm_out, HP32)
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(dg.cpu(), g), "grads are read-only"
        n32, _ = torch_step(p32, o32, g * grad_scale, max_norm, lr)       # a power of two: exact
        n64, _ = torch_step(p64, o64, g.double() * grad_scale, max_norm, lr)
        assert (float(n64) > max_norm * 1.1) if active else (float(n64) < max_norm * 0.9)
        m32, v32 = moments(o32, p32)
        m64, v64 = moments(o64, p64)
        for key, got, r32, r64 in (("p", dp.cpu(), p32.data, p64.data), ("m", dm.cpu(), m32, m64),
                                   ("v", dv.cpu(), v32, v64),
                                   ("norm", norm_out.cpu(), n32.reshape(1), n64.reshape(1))):
            d_ref = float((r32.double() - r64).abs().max())
            d_k = float((got.double() - r64).abs().max())
            ulp = float(np.spacing(np.float32(r64.abs().max())))
            bar = max(4.0 * d_ref, ulp)
            print(f"clip_adamw n={n} gs={grad_scale} active={active} step {step} {key}: kernel {d_k:.3e} "
                  f"torch fp32 {d_ref:.3e} ulp {ulp:.3e} bar {bar:.3e}")
            w = worst.setdefault(key, [0.0, 0.0, 0.0])
            if d_k / bar >= w[0]:
                worst[key] = [d_k / bar, d_k, bar, d_ref]
            assert d_k <= bar, (key, step, d_k, bar, d_ref)
        set_state(o64, p64, p32.data.double(), m32.double(), v32.double())   # next step from the fp32 state
    for key, w in worst.items():
        record("clip_adamw_fp32_vs_float64", f"n{n}_gs{grad_scale}_{'active' if active else 'inactive'}_{key}",
               kernel_dist=w[1], bar=w[2], torch_fp32_dist=w[3])


def test_clip_adamw_rejects_misaligned_grads(gpu):
    """grads is read as float4 by the norm pass: a pointer off 16 bytes is an error before any launch."""
    from projectiontrainer_amd import _lib as L
    host = [torch.randn(64) for _ in range(4)]
    dev = [t.to(gpu, copy=True) for t in host]
    norm_out = torch.full((1,), -7.0, dtype=torch.float32, device=gpu)
    for off in (1, 2, 3):
        rc = clip_adamw(dev[0][off:off + 40], dev[1][off:off + 40], dev[2][off:off + 40], dev[3][off:off + 40], 1.0,
                        5.0, 1e-3, 1, norm_out, HP32)
        assert rc != 0 and b"16-byte aligned" in L.lib().ptk_last_error()
    torch.cuda.synchronize()
    assert float(norm_out) == -7.0
    for a, b in zip(dev, host):
        assert torch.equal(a.cpu(), b)
    rc = clip_adamw(dev[0][off:off + 40], dev[1][4:44], dev[2][off:off + 40], dev[3][off:off + 40], 1.0, 5.0, 1e-3, 1,
                    norm_out, HP32)
    assert rc == 0   # only grads is vector-loaded
    torch.cuda.synchronize()
    assert float(norm_out) > 0.0
