"""One flat bf16 parameter store: what Stage 2's trained modules (Gemma3, projector, SigLIP tower) share.

Every parameter of a module lives in ONE flat bf16 buffer, the segments laid end to end and each rounded up to
`align` elements (64 = 128 B; the gaps stay zero); the grads in a second buffer of the same layout and, for a
store that owns its optimizer state, the two AdamW moments in two more.  Segments the kernels read in fp32
(norm weights, biases, positions) are listed as `mirrored`: they lie contiguously after the others, and one
fp32 buffer mirrors that region, refreshed by one copy after each optimizer step.  Saved optimizer shards
depend on the offsets and on `numel`.
"""
from __future__ import annotations

import math

import torch


class FlatStore:
    def __init__(self, segs, mirrored=(), *, device, align=64, pad_to=None, moments=False):
        """segs, mirrored: ordered (name, shape) lists.  pad_to: `numel` rounded up to a multiple of it (equal
        ZeRO shards).  moments: also allocate exp_avg, exp_avg_sq and the clip's sum-of-squares scalar."""
        segs, lo = list(segs), None
        off, self.offsets = 0, {}
        for j, (name, shape) in enumerate(segs + list(mirrored)):
            if j == len(segs):
                lo = off
            self.offsets[name] = (off, tuple(shape))
            off += (math.prod(shape) + align - 1) // align * align
        self.mirror_lo, self.mirror_hi = (off, off) if lo is None else (lo, off)
        self.numel = off if pad_to is None else (off + pad_to - 1) // pad_to * pad_to
        zeros = lambda: torch.zeros(self.numel, dtype=torch.bfloat16, device=device)
        self.flat, self.grad = zeros(), zeros()
        if moments:
            self.exp_avg, self.exp_avg_sq = zeros(), zeros()
            self.sumsq = torch.zeros(1, dtype=torch.float32, device=device)
        if lo is not None:
            self.mirror = torch.zeros(self.mirror_hi - lo, dtype=torch.float32, device=device)

    def view(self, name, buf=None):
        off, shape = self.offsets[name]
        return (self.flat if buf is None else buf)[off:off + math.prod(shape)].view(shape)

    def grad_view(self, name):
        return self.view(name, self.grad)

    def mirror_view(self, name):
        """The fp32 copy of a mirrored segment (a view of the mirror, current as of the last refresh_mirror)."""
        off, shape = self.offsets[name]
        return self.mirror[off - self.mirror_lo:][:math.prod(shape)].view(shape)

    def refresh_mirror(self):
        self.mirror.copy_(self.flat[self.mirror_lo:self.mirror_hi])

    def zero_grad(self):
        self.grad.zero_()
