"""Shared pieces of the loss-head tests (tests/test_loss_head_host.py, tests/test_loss_head_gpu.py): plain fp64
restatements on the CPU of what the lm_head statistics epilogue (gemm.hip), ce_stats_kernel / ce_kernel and the two
reductions (misc.hip) compute, the derived error bounds, and a generator of GEMM operands whose product is exact.
No kernel code is restated here: every function is the textbook definition in fp64.

The loss is ForCausalLMLoss (TF/loss/loss_utils.py:49-67): bf16 logits upcast, cross entropy with ignore_index -100,
mean over the valid targets.  Per row lse = log sum_c exp(x_c), loss = lse - x_target, and
d(logits)_c = (softmax_c - [c == target]) * g with g = loss_scale / count; an ignored row has loss 0 and gradient 0."""
import math

import torch

LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
EPS32 = 2.0 ** -23
F32_MIN_NORMAL = 2.0 ** -126
POISON_F32 = -12345.0
POISON_BF16 = 0x7A5C          # a finite bf16 (about 2.9e35) no kernel here produces
IGNORE = -100


def bits(t):
    return t.view(torch.int16)


def poison_bf16(rows, ld):
    return torch.full((rows, ld), POISON_BF16, dtype=torch.int16).view(torch.bfloat16)


def _floor_log2(x):
    """floor(log2 |x|) of an fp64 tensor, elementwise (0 maps to a very negative exponent)."""
    _, e = torch.frexp(x.double().abs())          # |x| = m 2^e, m in [0.5, 1)
    e = e.to(torch.int64) - 1
    return torch.where(x == 0, torch.full_like(e, -2000), e)


def ulp_bf16(x):
    """Spacing of bf16 (8 significand bits) at |x|, fp64: 2^(floor(log2 |x|) - 7), and 2^-133 below 2^-126."""
    return torch.pow(2.0, (_floor_log2(x).clamp(min=-126) - 7).double())


def ulp32(x):
    """Spacing of fp32 (24 significand bits) at |x|, fp64: 2^(floor(log2 |x|) - 23), and 2^-149 below 2^-126."""
    return torch.pow(2.0, (_floor_log2(x).clamp(min=-126) - 23).double())


def bf16_rne(x64):
    """fp64 -> bf16 by round-to-nearest-even.  Exact here only for values that fp32 holds exactly (the exact-operand
    products): the fp64 -> fp32 step is then the identity and the single rounding is fp32 -> bf16."""
    f = x64.float()
    assert torch.equal(f.double(), x64), "bf16_rne: the value is not an fp32 number (double rounding)"
    return f.bfloat16()


# ---------------------------------------------------------------- exact GEMM operands
def exact_operands(M, N, K, seed, big_rows=(), small_rows=()):
    """A [M][K], B [N][K] bf16 with entries that are multiples of 1/8 in [-2, 2] (33 values, 5 significant bits).
    Every product is a multiple of 1/64 of magnitude <= 4 and every partial sum over K <= 128 terms a multiple of
    1/64 of magnitude <= 512: 15 bits, so fp32 holds each partial sum exactly whatever the order, and the logits are
    exactly bf16_rne(A . B^T).  big_rows of A are scaled by 8 (integers up to 16; sums are multiples of 1/8 up to
    4096: 15 bits), which puts |logit| in the hundreds: exp(x) without the max subtraction overflows fp32.
    small_rows are scaled by 1/8 (multiples of 1/64 up to 1/4; sums are multiples of 1/512 up to 64: 15 bits): the
    logits crowd within a few units of the row maximum and many columns tie after the bf16 rounding."""
    assert K in (64, 128)
    g = torch.Generator().manual_seed(seed)
    A = torch.randint(-16, 17, (M, K), generator=g).double() / 8.0
    B = torch.randint(-16, 17, (N, K), generator=g).double() / 8.0
    for r in big_rows:
        A[r] *= 8.0
    for r in small_rows:
        A[r] /= 8.0
    A16, B16 = A.float().bfloat16(), B.float().bfloat16()
    assert torch.equal(A16.double(), A) and torch.equal(B16.double(), B)
    return A16, B16


def exact_logits(A16, B16):
    """(the fp64 product, its bf16 rounding): what any correct GEMM over exact_operands must store, bit for bit."""
    P = A16.double() @ B16.double().T
    return P, bf16_rne(P)


# ---------------------------------------------------------------- fp64 references
def chunk_stats_ref(logits, chunk=64):
    """Per row and `chunk` columns of bf16 logits [R][V]: (max [R][V / chunk], sum exp(x - max) [R][V / chunk]) in
    fp64.  A chunk that is all -inf has max -inf and sum NaN (-inf - -inf), as IEEE gives it."""
    R, V = logits.shape
    x = logits.double().view(R, V // chunk, chunk)
    m = x.max(dim=-1).values
    return m, torch.exp(x - m.unsqueeze(-1)).sum(dim=-1)


def lse_ref(logits):
    """Row log-sum-exp of bf16 logits [R][V] in fp64 (max-shifted; -inf entries contribute 0)."""
    x = logits.double()
    m = x.max(dim=-1, keepdim=True).values
    return (m + torch.log(torch.exp(x - m).sum(dim=-1, keepdim=True))).squeeze(-1)


def row_loss_ref(logits, targets):
    """fp64 loss per row: lse - x[target]; 0 for an ignored row (target < 0)."""
    lse = lse_ref(logits)
    valid = targets >= 0
    xt = logits.double().gather(1, targets.clamp(min=0).unsqueeze(1)).squeeze(1)
    return torch.where(valid, lse - xt, torch.zeros_like(lse))


def dlogits_ref(logits, targets, g):
    """(exact, allowance weight) in fp64: exact = (softmax - onehot) * g before any rounding, 0 on ignored rows; the
    weight p + [c == target] is what an fp32 relative error of the two terms scales with."""
    x = logits.double()
    p = torch.exp(x - lse_ref(logits).unsqueeze(-1))
    valid = (targets >= 0).unsqueeze(-1)
    onehot = torch.zeros_like(p)
    onehot.scatter_(1, targets.clamp(min=0).unsqueeze(1), 1.0)
    onehot = onehot * valid
    exact = torch.where(valid, (p - onehot) * g, torch.zeros_like(p))
    return exact, (p + onehot) * valid


def chunk_sum_bound(logits, chunk=64):
    """Bound on |stored sum - fp64 sum| of each chunk's sum exp(x - m), [R][V / chunk] fp64, from the data.

    The epilogue forms each term as e_i = exp2(fma(x_i, L2E, nm)) with nm = fl(-m L2E), m the chunk's exact maximum
    (exact: a maximum of bf16 values involves no rounding) and x_i the stored bf16 logit.  Against the true argument
    (x_i - m) log2(e), nm carries one rounding, at most ulp32(|m| L2E) / 2, and the fused multiply-add one more, at
    most ulp32(|x_i - m| L2E) / 2 (its result has that magnitude).  An argument error d changes 2^a by the factor
    2^d - 1 <= d ln 2 (1 + d): the term's error is e_i d_i ln 2.  The hardware exp2 is good to 1 ulp (2^-23
    relative), and a term passes through 6 fp32 additions on its way into the sum (3 levels inside the lane's 8
    columns, 3 DPP levels over the row's 8 lanes), each at most 2^-24 relative to a partial sum that never exceeds the
    total (all terms are positive): 2^-23 + 6 2^-24 = 2^-21 relative to the sum.  Hence

        bound = sum_i e_i ln 2 (ulp32(|m| L2E) / 2 + ulp32(|x_i - m| L2E) / 2) + 2^-21 sum_i e_i.

    The fp32 constant L2E is itself 1.3e-8 (2^-26.2) off log2(e), which moves an argument by less than half of its
    fma rounding term; it is not given a term of its own (the count of 8 roundings above is the worst case and the
    measured ratio shows the room).  Terms below the fp32 normal range (flushed to 0) are below 64 * 2^-126 in all,
    far under the 2^-21 the maximum's own term (e = 1) always contributes."""
    R, V = logits.shape
    x = logits.double().view(R, V // chunk, chunk)
    m = x.max(dim=-1, keepdim=True).values
    e = torch.exp(x - m)
    d = ulp32(m.abs() * LOG2E) / 2 + ulp32((x - m).abs() * LOG2E) / 2
    # (ulp32 of an exact 0, the maximum's own argument, is 2^-149: nothing)
    return (e * LN2 * d).sum(dim=-1) + 2.0 ** -21 * e.sum(dim=-1)


def dlogits_ok(got, exact, weight, g):
    """Elementwise: got (bf16) is a correctly rounded bf16 of an fp32 value within 1e-5 relative of the two terms,
    |got - exact| <= ulp_bf16(exact) / 2 + 1e-5 g (p + [c == target]); where |exact| is below the fp32 normal range
    a flushed 0 is accepted as well."""
    gd = got.double()
    err = (gd - exact).abs()
    bound = ulp_bf16(exact) / 2 + 1e-5 * abs(g) * weight
    return (err <= bound) | ((exact.abs() < F32_MIN_NORMAL) & (gd == 0))
