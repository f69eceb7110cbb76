"""References, input builders and checkers for the flash-attention kernel tests (tests/test_flash_exact_gpu.py;
self-tested on the CPU by tests/test_flash_checks_cpu.py).  No GPU dependency: everything here is plain torch
float64 and runs on whatever device its inputs live on.

Layout used throughout: Q, dO, O, dQ [Z, rows, D]; K, V, dK, dV [Z, nkeys, D]; LSE [Z, rows]; z = b * Hkv + kv head;
the G query heads of a kv head are the rows (s, j) -> s * G + j of one z, so a row's position is row // G.

Three ways to see a kernel fault:
  * readout operands (one-hot V / dO, Q = a I, K = a e_k): an output element IS one P or dS entry, so a wrong mask
    bit shows as a non-zero where an exact 0.0 belongs (check_zeros) or as a missing entry (check_readout);
  * per-row norms against the absolute-value companion of each output (check_rows);
  * LSE against the fp32 dot-product error bound (check_lse).

Bars.  E_* is the worst ratio of emulate() (the kernels' bf16 rounding points, otherwise float64) against
attn_ref64 over every case of the GPU file, measured by `python -m tests.flash_util` on the CPU; each bar is 4 E_*:
the factor covers fp32 summation order and v_exp / v_log error, which the emulation does not model."""
from types import SimpleNamespace

import torch

LOG2E = 1.4426950408889634
FA_DEFER = 8.0        # flash.hip: the running max moves only by more than this many log2 units

# measured worst emulation / float64 ratios (python -m tests.flash_util) and the bars = 4 x
E_ROWS = {"O": 6.9e-3, "dQ": 2.9e-3, "dK": 3.6e-3, "dV": 3.9e-3}
E_READ = {"O": 7.6e-3, "dQ": 7.2e-3, "dK": 7.3e-3, "dV": 3.9e-3}     # two bf16 roundings = 2^-7 = 7.8e-3 at worst
TAU = {k: 4 * v for k, v in E_ROWS.items()}      # check_rows: |got_r - ref_r| <= TAU |comp_r|
REL = {k: 4 * v for k, v in E_READ.items()}      # check_readout: |got - ref| <= REL comp + FLOOR
FLOOR = 2.0 ** -126                               # fp32 denormals may flush
# LSE: not an emulation bar (the emulation's LSE is exact up to its fp32 store).  The kernels accumulate a
# score's D products in fp32, |error| <= D 2^-24 sum|q_i k_i| scale (the standard dot-product bound, in nats as the
# LSE is); the exp / sum / log chain and the fp32 store add a few ulps of max(1, |LSE|): 2^-20 (1 + |LSE|).
LSE_ULPS = 2.0 ** -20
P_MIN = 1e-30         # readout inputs: no visible or would-be-leaked P below this (a leak cannot underflow to 0)


def bf16r(x):
    """Round to bf16 values, keeping the dtype."""
    return x.to(torch.bfloat16).to(x.dtype)


def mask(rows, nkeys, qdiv=1, causal=False, window=0, key_valid=None, key_len=None, diag=0, device=None):
    """FlashArgs' mask restated: [B or 1, rows, nkeys] bool.  position = row // qdiv; causal: k <= position;
    window (only under causal): k > position - window; key_valid [B, nkeys] (non-zero = valid) or key_len.
    diag shifts the causal diagonal (mutated references only)."""
    device = key_valid.device if key_valid is not None else device
    pos = (torch.arange(rows, device=device) // qdiv)[:, None]
    k = torch.arange(nkeys, device=device)[None, :]
    m = torch.ones(rows, nkeys, dtype=torch.bool, device=device)
    if causal:
        m = m & (k <= pos + diag)
        if window > 0:
            m = m & (k > pos - window)
    if key_valid is not None:
        return m[None] & (key_valid != 0)[:, None, :]
    if key_len is not None:
        m = m & (k < key_len)
    return m[None]


def attn_ref64(Q, K, V, dO, m, scale, drop=None):
    """float64 attention forward and backward on the given (bf16-valued) operands; m [Z, rows, nkeys] bool.
    Fully masked rows: P = 0, O = 0, LSE = -inf (the kernels' convention).  Every output comes with its
    absolute-value companion c*: cO = P |V|; cdQ = (P (|dP| + cdelta) scale) |K|, cdK its transpose form with |Q|,
    cdV = P^T |dO|, where cdelta = sum_i |dO_i| cO_i is delta's own companion.  (With |delta| in its place the
    companion misses the error delta inherits from the bf16 O, which scales with sum |dO| |P| |V| and not with the
    cancelled sum: rows with one dominant key then put the emulation at 0.28 of the companion, against 3e-3 here.)  drop = (z, r0, r1, k0, k1): rows [r0, r1) left out of dK / dV of keys [k0, k1)
    (a mutated reference: one query chunk dropped from one key slab)."""
    Q, K, V = Q.double(), K.double(), V.double()
    s = (Q @ K.transpose(-1, -2)) * scale
    s = s.masked_fill(~m, float("-inf"))
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse.masked_fill(torch.isinf(lse), 0.0)[..., None])     # masked: exp(-inf) = 0
    r = SimpleNamespace(S=s, P=P, LSE=lse, O=P @ V, cO=P @ V.abs(), cS=(Q.abs() @ K.abs().transpose(-1, -2)) * scale)
    if dO is None:
        return r
    dO = dO.double()
    delta = (dO * r.O).sum(-1, keepdim=True)
    dP = dO @ V.transpose(-1, -2)
    dS = P * (dP - delta)
    cdS = P * (dP.abs() + (dO.abs() * r.cO).sum(-1, keepdim=True)) * scale
    r.dS, r.dQ, r.cdQ = dS, (dS @ K) * scale, cdS @ K.abs()
    Pt, dSt, cdSt = P, dS, cdS
    if drop is not None:
        z, r0, r1, k0, k1 = drop
        Pt, dSt, cdSt = P.clone(), dS.clone(), cdS.clone()
        for t in (Pt, dSt, cdSt):
            t[z, r0:r1, k0:k1] = 0
    r.dK, r.cdK = (dSt.transpose(-1, -2) @ Q) * scale, cdSt.transpose(-1, -2) @ Q.abs()
    r.dV, r.cdV = Pt.transpose(-1, -2) @ dO, Pt.transpose(-1, -2) @ dO.abs()
    return r


def _online(s, m, sl2, tile, on_tile):
    """The kernels' online-softmax walk over key tiles of raw scores s: the running max moves only when a tile's
    max exceeds it by more than FA_DEFER log2 units (`up = mt > m_run + 8 / sl2`).  Calls
    on_tile(t0, st, mc, alpha, event, events so far) per tile; returns (m_run, events per row after the first tile)."""
    thr = FA_DEFER / sl2
    m_run = torch.full(s.shape[:-1], float("-inf"), dtype=s.dtype, device=s.device)
    events = torch.zeros(s.shape[:-1], dtype=torch.long, device=s.device)
    for t0 in range(0, s.shape[-1], tile):
        st = s[..., t0:t0 + tile].masked_fill(~m[..., t0:t0 + tile], float("-inf"))
        mt = st.amax(-1)
        up = mt > m_run + thr                      # m_run = -inf: any finite tile max moves it
        m_new = torch.where(up, mt, m_run)
        ev = up & torch.isfinite(m_run)
        alpha = torch.where(ev, torch.exp2((m_run - m_new).nan_to_num(nan=0.0, neginf=0.0) * sl2), torch.ones_like(mt))
        mc = torch.where(torch.isinf(m_new), torch.zeros_like(mt), m_new * sl2)
        on_tile(t0, st, mc, alpha, ev, events)
        events = events + ev.long()
        m_run = m_new
    return m_run, events


def rescale_events(scores, m, tile, scale=1.0):
    """Rescale events (alpha != 1) per row under the deferred-max rule at key tiles of `tile`, for raw scores
    [.., rows, nkeys] that the kernel multiplies by `scale`."""
    return _online(scores.double(), m, scale * LOG2E, tile, lambda *a: None)[1]


def emulate(Q, K, V, dO, m, scale, tile=32, skip_alpha=None):
    """attn_ref64's computation with the kernels' rounding points, taken from flash.hip: the online-softmax
    forward with the deferred max, P to bf16 before P V (the row sum adds the unrounded P), O to bf16; backward:
    LSE as stored (fp32), P to bf16 before dV and dS, O (bf16) in delta, dS to bf16 before dQ and dK, outputs to
    bf16.  Everything else is float64.  skip_alpha = (z, row, n): the O rescale of that row's n-th event is
    skipped (a mutation for the self-test)."""
    Q, K, V = Q.double(), K.double(), V.double()
    s = Q @ K.transpose(-1, -2)
    sl2 = scale * LOG2E
    acc = SimpleNamespace(O=torch.zeros_like(Q[..., :1] * V[..., :1, :]), l=torch.zeros_like(s[..., 0]))

    def on_tile(t0, st, mc, alpha, ev, events):
        p = torch.exp2(st * sl2 - mc[..., None])
        a_o = alpha
        if skip_alpha is not None:
            z, row, n = skip_alpha
            if bool(ev[z, row]) and int(events[z, row]) == n:
                a_o = alpha.clone()
                a_o[z, row] = 1.0
        acc.l = acc.l * alpha + p.sum(-1)
        acc.O = acc.O * a_o[..., None] + bf16r(p) @ V[..., t0:t0 + st.shape[-1], :]

    m_run, events = _online(s, m, sl2, tile, on_tile)
    live = acc.l > 0
    inv = torch.where(live, 1.0 / acc.l.clamp_min(1e-300), torch.zeros_like(acc.l))
    r = SimpleNamespace(events=events, O=bf16r(acc.O * inv[..., None]))
    lse = (torch.where(live, m_run, torch.zeros_like(m_run)) * sl2 + torch.log2(acc.l.clamp_min(1e-300))) / LOG2E
    r.LSE = torch.where(live, lse.float().double(), torch.full_like(lse, float("-inf")))
    if dO is None:
        return r
    dO = dO.double()
    Pb = bf16r(torch.exp((s * scale).masked_fill(~m, float("-inf")) - r.LSE.masked_fill(~live, 0.0)[..., None]))
    delta = (dO * r.O).sum(-1, keepdim=True)
    dS = bf16r(Pb * (dO @ V.transpose(-1, -2) - delta))
    r.dQ = bf16r((dS @ K) * scale)
    r.dK = bf16r((dS.transpose(-1, -2) @ Q) * scale)
    r.dV = bf16r(Pb.transpose(-1, -2) @ dO)
    return r


# ------------------------------------------------------------------------------------------------ checkers
def _fail(name, what, idx, got, ref, bound):
    raise AssertionError(f"{name}: {what} at {tuple(int(i) for i in idx)}: got {float(got)!r}, ref {float(ref)!r}, "
                         f"bound {float(bound)!r}")


def support(A, B):
    """True where sum_j |A[.., i, j]| |B[.., j, c]| has a non-zero term: the output elements that receive any
    contribution at all (A: a bool mask or an operand)."""
    return ((A != 0).double() @ (B != 0).double()) > 0


def check_zeros(got, sup, name="zeros"):
    """Exact 0.0 wherever the reference mask lets no term contribute: masked P is exp2(-inf) = 0 and zeros add
    exactly, so any other value is a leaked key.  Returns the number of elements checked."""
    bad = (got.double() != 0) & ~sup
    if bool(bad.any()):
        idx = bad.nonzero()[0]
        _fail(name, f"{int(bad.sum())} non-zero element(s) where no key contributes, first", idx, got[tuple(idx)], 0.0, 0.0)
    return int((~sup).sum())


def check_readout(got, ref, comp, rel, name="readout", floor=FLOOR):
    """Elementwise |got - ref| <= rel comp + floor.  Returns the worst |got - ref| / (comp + floor / rel)."""
    err = (got.double() - ref).abs()
    ratio = err / (comp + floor / rel)
    if not bool(torch.isfinite(got.double()).all()):
        raise AssertionError(f"{name}: non-finite output")
    worst = float(ratio.max())
    if worst > rel:
        idx = (ratio == ratio.max()).nonzero()[0]
        _fail(name, f"ratio {worst:.3e} > {rel:.3e}", idx, got[tuple(idx)], ref[tuple(idx)], rel * comp[tuple(idx)] + floor)
    return worst


def check_rows(got, ref, comp, tau, name="rows"):
    """Per output row r (every z): ||got_r - ref_r|| <= tau ||comp_r||; rows whose companion is 0 receive no
    contribution and must be exactly 0.  Returns the worst ratio."""
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        raise AssertionError(f"{name}: non-finite output")
    err = (got - ref).norm(dim=-1)
    cn = comp.norm(dim=-1)
    dead = cn == 0
    if bool((err[dead] != 0).any()):
        idx = ((err != 0) & dead).nonzero()[0]
        _fail(name, "row with no contribution is not zero", idx, err[tuple(idx)], 0.0, 0.0)
    ratio = torch.where(dead, torch.zeros_like(err), err / cn.clamp_min(1e-300))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if worst > tau:
        idx = (ratio == ratio.max()).nonzero()[0]
        _fail(name, f"row ratio {worst:.3e} > {tau:.3e} ({int((ratio > tau).sum())} rows over)", idx, err[tuple(idx)], 0.0,
              tau * cn[tuple(idx)])
    return worst


def check_lse(got, ref, cS, m, D, name="LSE", scale_bound=1.0):
    """-inf exactly where the row is fully masked; elsewhere |got - ref| <= D 2^-24 max_k cS[q, k] (visible k)
    + LSE_ULPS (1 + |ref|).  Returns the worst error / bound (scale_bound scales the bound: the self-test's half)."""
    got = got.double()
    dead = torch.isinf(ref)
    if not bool((got[dead] == ref[dead]).all()):
        idx = (dead & (got != ref)).nonzero()[0]
        _fail(name, "fully masked row", idx, got[tuple(idx)], ref[tuple(idx)], 0.0)
    bound = D * 2.0 ** -24 * cS.masked_fill(~m, 0.0).amax(-1) + LSE_ULPS * (1 + ref.masked_fill(dead, 0.0).abs())
    ratio = torch.where(dead, torch.zeros_like(ref), (got - ref).abs() / bound)
    if bool(torch.isnan(ratio).any()) or bool(torch.isinf(got[~dead]).any()):
        raise AssertionError(f"{name}: non-finite value on a live row")
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if worst > scale_bound:
        idx = (ratio == ratio.max()).nonzero()[0]
        _fail(name, f"ratio {worst:.3e} > {scale_bound}", idx, got[tuple(idx)], ref[tuple(idx)], bound[tuple(idx)])
    return worst


# ------------------------------------------------------------------------------------------------ inputs
def _randn(*shape, seed, mul=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * mul).to(torch.bfloat16)


def one_hot_rows(Z, n, D, first=0):
    """[Z, n, D] bf16 with row k = e_{(first + k) mod D}."""
    x = torch.zeros(Z, n, D, dtype=torch.bfloat16)
    k = torch.arange(n)
    x[:, k, (first + k) % D] = 1
    return x


def key_valid_std(B, S):
    """The family's key padding: even samples left-padded (70 keys = two whole 32-key tiles + 6 from S 128 on, 6 keys
    below), odd samples with a hole ([200, 215) from S 256 on) and their tail invalid; further samples shift both."""
    kv = torch.ones(B, S, dtype=torch.int32)
    pad = 70 if S >= 128 else 6
    lo, n, tail = (200, 15, 30) if S >= 256 else (S // 2 + 3, 3, 4)
    for b in range(B):
        if b % 2 == 0:
            kv[b, :pad + 4 * (b // 2)] = 0
        else:
            kv[b, lo + b // 2:lo + b // 2 + n] = 0
            kv[b, S - tail:] = 0
    return kv


def case(name, D, Hkv, G, Q, K, V, dO=None, causal=False, window=0, key_valid=None, tile=None, **extra):
    """A test case: operands in the module's layout plus the FlashArgs mask fields."""
    Z, rows, nkeys = Q.shape[0], Q.shape[1], K.shape[1]
    return SimpleNamespace(name=name, D=D, Hkv=Hkv, G=G, Z=Z, B=Z // Hkv, rows=rows, nkeys=nkeys, Q=Q, K=K, V=V, dO=dO,
                           causal=causal, window=window, key_valid=key_valid, scale=D ** -0.5,
                           tile=tile or (32 if D == 256 else 64), **extra)


def case_mask(c, device=None, **mut):
    """[Z, rows, nkeys] mask of a case (mut: mask() overrides for mutated references)."""
    kv = c.key_valid if c.key_valid is None or device is None else c.key_valid.to(device)
    a = dict(qdiv=c.G, causal=c.causal, window=c.window, key_valid=kv, device=device)
    a.update(mut)
    m = mask(c.rows, c.nkeys, **a)
    return m.repeat_interleave(c.Hkv, 0) if m.shape[0] > 1 else m.expand(c.Z, -1, -1)


def to(c, device):
    """The case with its tensors on `device`."""
    d = dict(vars(c))
    for k, v in d.items():
        if torch.is_tensor(v):
            d[k] = v.to(device)
    return SimpleNamespace(**d)


def ref_of(c, **kw):
    return attn_ref64(c.Q, c.K, c.V, c.dO, case_mask(c, c.Q.device), c.scale, **kw)


def emu_of(c, m=None, **kw):
    return emulate(c.Q, c.K, c.V, c.dO, case_mask(c, c.Q.device) if m is None else m, c.scale, tile=c.tile, **kw)


def fwd_readout_case(D, Hkv, G, S, B, window, causal=True, nkeys=None, rows=None, key_valid="std", seed=100):
    """V one-hot (V[k] = e_{k mod D}): O[q][c] = sum of P[q, k] over k = c (mod D).  Q is N(0, 1) x 3, so scores
    have std 3 nats and no P underflows."""
    rows = S * G if rows is None else rows
    nkeys = S if nkeys is None else nkeys
    Z = B * Hkv
    kv = key_valid_std(B, nkeys) if isinstance(key_valid, str) else key_valid
    return case(f"fwd_readout D{D} Hkv{Hkv} G{G} rows{rows} keys{nkeys} B{B} W{window} c{int(causal)}", D, Hkv, G,
                _randn(Z, rows, D, seed=seed, mul=3.0), _randn(Z, nkeys, D, seed=seed + 1), one_hot_rows(Z, nkeys, D),
                causal=causal, window=window, key_valid=kv)


def generic_fwd_case():
    """Past the 4096-key mask table (the generic forward kernel): rows 128, 4128 keys, G 1, non-causal; the keys of
    classes 0..7 (k mod 256 < 8) and the first 70 keys are invalid, so those 8 classes read exact zeros and the
    others fold 15 to 17 keys each."""
    kv = torch.ones(1, 4128, dtype=torch.int32)
    kv[0, :70] = 0
    kv[0, torch.arange(4128) % 256 < 8] = 0
    return fwd_readout_case(256, 1, 1, 128, 1, 0, causal=False, nkeys=4128, rows=128, key_valid=kv, seed=110)


def decode_case(G, nkeys, with_kv, Hkv=2, B=2, D=256, offset=40, tail=24, seed=120):
    """A decode step: rows = G, non-causal, K / V views at `offset` into a cache of offset + nkeys + tail rows.
    Real keys carry V classes 0 .. min(nkeys, D - 16) - 1; every cache row outside the view is bait: K = 4 x the
    mean query row (a score that would dominate every row's) and V in a class no real key uses (D - 16 ..)."""
    Z = B * Hkv
    Q = _randn(Z, G, D, seed=seed, mul=3.0)
    Smax = offset + nkeys + tail
    kc = Q.float().mean(1, keepdim=True).mul(4.0).to(torch.bfloat16).expand(Z, Smax, D).clone()
    vc = torch.zeros(Z, Smax, D, dtype=torch.bfloat16)
    vc[:, torch.arange(Smax), D - 16 + torch.arange(Smax) % 16] = 1
    kc[:, offset:offset + nkeys] = _randn(Z, nkeys, D, seed=seed + 1)
    vc[:, offset:offset + nkeys] = 0
    k = torch.arange(nkeys)
    vc[:, offset + k, k % (D - 16)] = 1
    kv = None
    if with_kv:    # per sample: leading slots off (left-padded prompt), a hole, sample 1 its last 4 keys off
        kv = torch.ones(B, nkeys, dtype=torch.int32)
        kv[0, :min(9, nkeys // 4)] = 0
        kv[1, nkeys // 2:nkeys // 2 + 3] = 0
        kv[1, nkeys - 4:] = 0
    c = case(f"decode G{G} keys{nkeys} kv{int(with_kv)}", D, Hkv, G, Q, kc[:, offset:offset + nkeys], vc[:, offset:offset + nkeys],
             key_valid=kv, Kcache=kc, Vcache=vc, offset=offset)
    return c


def _grid_scores(Z, rows, nkeys, seed, lo=-24, hi=24):
    """Scores that are multiples of 1/8 (here within +-3 nats): exact in bf16 up to magnitude 31."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(lo, hi + 1, (Z, rows, nkeys), generator=g).double() / 8


def scores_case(name, D, Hkv, G, scores, kind="qI", seed=130, **kw):
    """Operands whose score matrix is `scores` [Z, rows, nkeys] exactly (entries multiples of 1/8, |.| <= 31), with
    a = D^0.5 so that a scale = 1:
      kind "qI": Q = a I (rows <= D), K[k][q] = scores[q, k]: dK[k][q] = dS[q, k];
      kind "kI": K = a e_k (nkeys <= D), Q[q][k] = scores[q, k]: dQ[q][k] = dS[q, k].
    dO is one-hot by row when rows <= D (dV[k][q] = P[q, k]) unless kw gives random dO; V is N(0, 1)."""
    Z, rows, nkeys = scores.shape
    a = D ** 0.5
    assert float(scores.abs().max()) <= 31 and bool(((scores * 8) == (scores * 8).round()).all())
    if kind == "qI":
        assert rows <= D
        Q = torch.zeros(Z, rows, D, dtype=torch.bfloat16)
        Q[:, torch.arange(rows), torch.arange(rows)] = a
        K = torch.zeros(Z, nkeys, D, dtype=torch.bfloat16)
        K[:, :, :rows] = scores.transpose(1, 2).to(torch.bfloat16)
    else:
        assert nkeys <= D
        K = torch.zeros(Z, nkeys, D, dtype=torch.bfloat16)
        K[:, torch.arange(nkeys), torch.arange(nkeys)] = a
        Q = torch.zeros(Z, rows, D, dtype=torch.bfloat16)
        Q[:, :, :nkeys] = scores.to(torch.bfloat16)
    random_do = kw.pop("random_do", False)
    dO = _randn(Z, rows, D, seed=seed + 2) if random_do else one_hot_rows(Z, rows, D)
    return case(name, D, Hkv, G, Q, K, _randn(Z, nkeys, D, seed=seed + 1), dO, kind=kind, **kw)


def bwd_readout_case(D, S, G, window, kind="qI", B=2, seed=140):
    """F5: causal GQA with left padding and a hole, scores on the 1/8 grid within +-3 nats."""
    sc = _grid_scores(B, S * G, S, seed)
    return scores_case(f"bwd_readout {kind} D{D} S{S} G{G} W{window}", D, 1, G, sc, kind=kind, seed=seed, causal=True,
                       window=window, key_valid=key_valid_std(B, S))


def dynrange_scores(rows, nkeys, tile, causal, shift=0):
    """F4 score rows by (q + shift) mod 4, in nats on the 1/8 grid (8 log2 units = 5.545 nats):
      0  a staircase of +6.25 nats (9.02 log2 units) per tile: a rescale at every tile;
      1  steps of +5.5 (7.93 log2) then +0.25 (0.36 log2): under FA_DEFER, then over it counted from the last move;
      2  monotone decreasing (never a rescale);
      3  flat, with a +27.75 nat (40 log2) spike on the last visible key."""
    k = torch.arange(nkeys)
    t = k // tile
    nt = (nkeys + tile - 1) // tile
    s = torch.zeros(rows, nkeys, dtype=torch.float64)
    for q in range(rows):
        jit = -((k * 7 + q) % 8).double() / 8
        pat = (q + shift) % 4
        if pat == 0:
            s[q] = -6.25 * (nt - 1) / 2 - 0.125 * ((nt - 1) % 2) + 6.25 * t + jit
        elif pat == 1:
            s[q] = -15.0 + 5.5 * ((t + 1) // 2) + 0.25 * (t // 2) - ((k + q) % 2).double() / 8
        elif pat == 2:
            s[q] = 20.0 - (k * min(320, nkeys) // nkeys).double() / 8
        else:
            s[q] = -14.0 + jit
            s[q, min(q, nkeys - 1) if causal else nkeys - 1] = 13.75
    return s


def dynrange_case(D, causal, nkeys=320, Z=2, seed=150):
    """F4: Q = a I, rows = D (256 or 64), V and dO random; z takes the row patterns shifted by z."""
    tile = 32 if D == 256 else 64
    sc = torch.stack([dynrange_scores(D, nkeys, tile, causal, shift=z) for z in range(Z)])
    return scores_case(f"dynrange D{D} keys{nkeys} c{int(causal)}", D, 1, 1, sc, kind="qI", seed=seed, causal=causal,
                       random_do=True)


def random_case(D, Hkv, G, S, B, window, key_valid="std", seed=160, name="random"):
    """F6 / F7: Q N(0, 1) x 3, K, V, dO N(0, 1), causal."""
    Z = B * Hkv
    kv = key_valid_std(B, S) if isinstance(key_valid, str) else key_valid
    return case(f"{name} D{D} Hkv{Hkv} G{G} S{S} B{B} W{window}", D, Hkv, G, _randn(Z, S * G, D, seed=seed, mul=3.0),
                _randn(Z, S, D, seed=seed + 1), _randn(Z, S, D, seed=seed + 2), _randn(Z, S * G, D, seed=seed + 3),
                causal=True, window=window, key_valid=kv)


def persist_key_valid(B, S=64):
    """F6: a distinct key_valid row per sample: b % 23 leading keys off, one hole of 1 + b % 3 keys at 30 + b % 29."""
    kv = torch.ones(B, S, dtype=torch.int32)
    for b in range(B):
        kv[b, :b % 23] = 0
        kv[b, 30 + b % 29:30 + b % 29 + 1 + b % 3] = 0
    return kv


def persist_case(B, window):
    return random_case(256, 2, 4, 64, B, window, key_valid=persist_key_valid(B), seed=170, name="persist")


# ---- the case lists of the GPU file (shared with the self-test and the bar measurement)
F1_WINDOWS = (1, 2, 31, 32, 33, 63, 64, 65, 100, 255, 256, 0)
F1_SHAPES = ((4, 320), (3, 300), (1, 36))                     # (G, S)
F2_N = (4, 63, 64, 65, 196)
F2_WINDOWS = (1, 63, 64)
F3_G = (1, 4, 8)
F3_NKEYS = (4, 5, 31, 32, 33, 255, 333)
F3_NKEYS_KV = (32, 36, 332)
# (D, causal, nkeys).  hd 64 walks 64-key tiles: 320 keys are 5 tiles (at most 4 rescales), so a 512-key case is added
# for the >= 6 events; its causal case (64 rows, G 1) stays inside one tile and rescales nothing.
F4_CASES = ((256, True, 320), (256, False, 320), (64, True, 320), (64, False, 320), (64, False, 512))
F5_SHAPES = ((256, 256, 1), (256, 128, 2), (256, 64, 4), (256, 64, 3), (64, 64, 1))                    # (D, S, G)
F5_DUAL = ((256, 256, 1), (256, 128, 2), (256, 64, 4))
F5_WINDOWS = (0, 1, 32, 33, 100)
F6_WINDOWS = (0, 33)
F7_CASES = ((704, 512, 2), (704, 0, 2), (1088, 512, 1))       # (S, window, B)


def f1_case(G, S, window):
    return fwd_readout_case(256, 1, G, S, 2, window)


def f2_case(N=None, window=None):
    """hd 64 (tile 64): non-causal N keys, B 2 x 4 heads (the fused qkv layout), or causal G 2 / S 128 with key_valid."""
    if N is not None:
        return fwd_readout_case(64, 4, 1, N, 2, 0, causal=False, key_valid=None, seed=180)
    return fwd_readout_case(64, 1, 2, 128, 2, window, seed=181)


def all_cases(persist_B=80):
    """(family, case, has readout outputs) of every case the GPU file runs (F6 at the B of a 256-CU device)."""
    for G, S in F1_SHAPES:
        for w in (F1_WINDOWS if S == 320 else (0, 33)):
            yield "F1", f1_case(G, S, w)
    yield "F1", generic_fwd_case()
    for N in F2_N:
        yield "F2", f2_case(N=N)
    for w in F2_WINDOWS:
        yield "F2", f2_case(window=w)
    for G in F3_G:
        for n in F3_NKEYS:
            yield "F3", decode_case(G, n, False)
        for n in F3_NKEYS_KV:
            yield "F3", decode_case(G, n, True)
    for D, causal, n in F4_CASES:
        yield "F4", dynrange_case(D, causal, n)
    for D, S, G in F5_SHAPES:
        for w in F5_WINDOWS:
            yield "F5", bwd_readout_case(D, S, G, w)
    for D, S, G in F5_DUAL:
        for w in F5_WINDOWS:
            yield "F5", bwd_readout_case(D, S, G, w, kind="kI")
    for w in F6_WINDOWS:
        yield "F6", persist_case(persist_B, w)
    for S, w, B in F7_CASES:
        yield "F7", random_case(256, 1, 4, S, B, w)


def check_family(fam, c, ref, got, m, frac=1.0, lse=True):
    """Every check of a family on the outputs `got` holds (O, LSE, dQ, dK, dV; absent ones are skipped), at `frac` of
    the bars: exact zeros and per-row norms on every output, element readout on the family's readout outputs, LSE.
    Returns the worst ratios, keyed "rows O", "read dK", "LSE", .."""
    out = {}
    Q, K, V = c.Q.double(), c.K.double(), c.V.double()
    mt = m.transpose(-1, -2)
    sup = {"O": lambda: support(m, V), "dQ": lambda: support(m, K), "dK": lambda: support(mt, Q),
           "dV": lambda: support(mt, c.dO.double())}
    for k in ("O", "dQ", "dK", "dV"):
        g = getattr(got, k, None)
        if g is None:
            continue
        check_zeros(g, sup[k](), f"{c.name} {k}")
        if k in readout_outputs(fam, c):
            out["read " + k] = check_readout(g, getattr(ref, k), getattr(ref, "c" + k), REL[k] * frac, f"{c.name} {k}")
        out["rows " + k] = check_rows(g, getattr(ref, k), getattr(ref, "c" + k), TAU[k] * frac, f"{c.name} {k}")
    if lse and getattr(got, "LSE", None) is not None:
        out["LSE"] = check_lse(got.LSE, ref.LSE, ref.cS, m, c.D, f"{c.name} LSE", scale_bound=frac)
    return out


READOUT = {"F1": ("O",), "F2": ("O",), "F3": ("O",), "F5": ("dK", "dV", "dQ")}


def readout_outputs(fam, c):
    """The outputs of a case that read out P or dS elementwise."""
    if fam == "F5":
        return ("dK", "dV") if c.kind == "qI" else ("dQ", "dV")
    return READOUT.get(fam, ())


def ratios(ref, got, kinds, what):
    """Worst row ratios (what = "rows") or element ratios ("read") of got against ref per output kind."""
    out = {}
    for k in kinds:
        r, g, c = getattr(ref, k), getattr(got, k).double(), getattr(ref, "c" + k)
        if what == "rows":
            cn = c.norm(dim=-1)
            out[k] = float(((g - r).norm(dim=-1) / cn.clamp_min(1e-300))[cn > 0].max())
        else:
            out[k] = float(((g - r).abs() / (c + FLOOR))[c > 0].max())
    return out


def measure():
    """The worst emulation / float64 ratios over every GPU case: the E_* constants above."""
    rows, read = {}, {}
    for fam, c in all_cases():
        ref, emu = ref_of(c), emu_of(c)
        kinds = ("O",) if c.dO is None else ("O", "dQ", "dK", "dV")
        rr = ratios(ref, emu, kinds, "rows")
        ro = ratios(ref, emu, readout_outputs(fam, c), "read")
        print(f"{fam} {c.name}: rows {rr} read {ro}", flush=True)
        for k, v in rr.items():
            rows[k] = max(rows.get(k, 0.0), v)
        for k, v in ro.items():
            read[k] = max(read.get(k, 0.0), v)
    print("E_ROWS =", {k: float(f"{v:.3e}") for k, v in rows.items()})
    print("E_READ =", {k: float(f"{v:.3e}") for k, v in read.items()})


if __name__ == "__main__":
    measure()
