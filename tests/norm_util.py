"""Shared pieces of the norm-kernel tests (tests/test_norm_kernels_gpu.py, tests/test_norm_wgrad_gpu.py): plain fp64
references on the CPU, the derived error bound, NaN padding and canaries.

Gemma3RMSNorm is TF/models/gemma3/modeling_gemma3.py:136-150 (fp32 math, rstd = rsqrt(mean(x^2) + eps), scale
1 + w, cast to the input dtype); the sandwich placement is :399-429.

The bound.  For an output whose exact value is r = sum of terms, M is the sum of the terms' magnitudes and the
kernel's fp32 value may differ from r by at most REL * M with REL = 2^-17: at most 48 sequential adds per lane at
cols = 3072, 6 butterfly steps, under ten multiplies / adds and the rsqrt are about 62 roundings of 2^-24, doubled.
The weight-grad sums stay under the same count (8 + 3 per 32-row block, 4 + 3 per 16-row fold, 16 + 15 in the finish).
A bf16 output must lie in [bf16(r - d), bf16(r + d)]: rounding is monotone, so the interval is exact, and where its
ends coincide it is bit equality."""
import torch

REL = 2.0 ** -17
CANARY_F32 = -12345.0
CANARY_BF16 = 0x7A5C          # a finite bf16 no kernel here produces
CANARY_BITS = torch.tensor(CANARY_BF16, dtype=torch.int16)


def bfr(x):
    """Round to bf16, returned in the dtype given.  An fp64 value goes through fp32 first: the kernels round fp32
    values, and for every fp32 v >= lo the chain bf16(fp32(lo)) <= bf16(v) holds (both roundings are monotone)."""
    return x.float().bfloat16().to(x.dtype)


def bits(t):
    return t.view(torch.int16)


def rstd_ref(x, eps):
    """fp64 rstd per row."""
    x = x.double()
    return torch.rsqrt((x * x).mean(dim=-1) + eps)


def rms_bwd_ref(x, w, rstd, dn):
    """(dx, M) in fp64: dx = dn (1+w) rs - x rs^3 sum(dn (1+w) x) / cols, M the sum of the magnitudes of its terms."""
    x, dn, rs = x.double(), dn.double(), rstd.double().unsqueeze(-1)
    g = dn * (1.0 + w.double())
    cols = x.shape[-1]
    dot = (g * x).sum(dim=-1, keepdim=True)
    adot = (g * x).abs().sum(dim=-1, keepdim=True)
    dx = g * rs - x * rs ** 3 * dot / cols
    M = g.abs() * rs + x.abs() * rs ** 3 * adot / cols
    return dx, M


def bf16_interval(r, d):
    """[lo, hi] (fp64 tensors holding bf16 values) that a bf16 output with exact value r and fp32 error <= d lies in."""
    return bfr(r - d), bfr(r + d)


def single_valued(lo, hi):
    return float((lo == hi).double().mean())


def inside(got, lo, hi):
    """Elementwise lo <= got <= hi; a NaN in got is outside."""
    got = got.double()
    return (got >= lo) & (got <= hi)


def acc_interval(g0, S, d):
    """bf16(g0 + bf16(S +- d)) evaluated as the kernel does: bf16 round, one fp32 add, bf16 round (all monotone)."""
    g0 = g0.float()
    lo = (g0 + (S - d).float().bfloat16().float()).bfloat16()
    hi = (g0 + (S + d).float().bfloat16().float()).bfloat16()
    return lo.double(), hi.double()


def map_rows(m, rows):
    """Source rows of a row map (g, skip, gs, off) with skip == 0, as include/ptk.h defines it."""
    g, skip, gs, off = m
    r = torch.arange(rows)
    return r + off if g == 0 else (r // g) * gs + r % g + off


def padded(t, extra_rows=3, ld=None, fill=float("nan")):
    """A copy of the 2-D tensor t inside a [rows + extra_rows][ld] buffer filled with `fill` (NaN: a read past rows or
    past cols shows)."""
    rows, cols = t.shape
    ld = cols if ld is None else ld
    out = torch.full((rows + extra_rows, ld), fill, dtype=t.dtype)
    out[:rows, :cols] = t
    return out


def nonzero_g0(cols, gen, scale=1.0):
    """A non-zero, sign-mixed bf16 grad to accumulate into."""
    g = (torch.randint(1, 5, (cols,), generator=gen).float() * scale)
    g[torch.rand(cols, generator=gen) < 0.5] *= -1
    return g.bfloat16()
