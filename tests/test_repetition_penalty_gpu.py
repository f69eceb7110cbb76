"""Repetition penalty in both decoders on the GPU (ptk_sample_next_token, ptk_beam_candidates_penalized,
ptk_gemma3_generate_penalized; Gemma3CausalLM.generate / beam_candidates / beam_generate).

The reference everywhere is transformers' own RepetitionPenaltyLogitsProcessor on the CPU over fp32(bf16 logits):
on the raw logits ahead of the warpers for sampling and greedy (GenerationMixin._sample), on log_softmax of the
raw logits ahead of the warpers in beam search (_beam_search; nothing renormalised), chained with
oracle.beam_ref.processed_log_probs for the warpers.  processed_log_probs takes log_softmax of its input first, i.e.
subtracts c = logsumexp(input) per row; the warpers commute with that shift (top-k and top-p see differences and
ratios only), so for the unnormalised penalised log probs the chain is processed_log_probs(pen) + c / T.

Histories hold each row's raw top-4 tokens (so the penalty moves the head of the row), random tokens and a
repeated token (penalised once, as HF gathers then scatters).  The score bar is 2e-4 x max(1, p): 2e-4 is
tests/test_beam_gpu.py's bar for a log prob, and a penalised log prob carries the lse error times p."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_beam_gpu import _distinct_logits, _model

pytestmark = pytest.mark.gpu

BEAM_SCORES = [0.0, -0.7, -1.3]


def hf_penalise(hist, scores, p):
    from transformers.generation.logits_process import RepetitionPenaltyLogitsProcessor
    if hist is None or hist.shape[1] == 0 or p == 1.0:
        return scores.float()
    return RepetitionPenaltyLogitsProcessor(penalty=float(p))(hist.long(), scores.float().clone())


def history(lg, n, seed):
    """[rows, n]: the row's raw top-4 (as many as fit), random tokens, and the first token once more at the end."""
    rows, V = lg.shape
    h = torch.randint(0, V, (rows, n), generator=torch.Generator().manual_seed(seed))
    m = min(4, n)
    h[:, :m] = lg.float().topk(4, -1).indices[:, :m]
    if n >= 6:
        h[:, -1] = h[:, 0]
    return h


def ref_beam_log_probs(lg, hist, p, do_sample=False, top_k=0, top_p=1.0, temperature=1.0, min_keep=1):
    from oracle import beam_ref as BR
    pen = hf_penalise(hist, F.log_softmax(lg.float(), -1), p)
    if not do_sample:
        return pen
    c = torch.logsumexp(pen, -1, keepdim=True)
    return BR.processed_log_probs(pen, True, top_k, top_p, temperature, min_keep) + c / temperature


def ref_beam_candidates(lg, bs, K, n_cand, hist, p, **kw):
    V = lg.shape[-1]
    acc = (ref_beam_log_probs(lg, hist, p, **kw) + bs.float()[:, None]).reshape(-1, K * V)
    val, idx = torch.topk(acc, n_cand, -1)
    return idx % V, idx // V, val, acc


def pinned_places(rs):
    """[B, n] of reference scores [B, n + 1]: places more than 1e-3 away from both neighbours."""
    apart = (rs[:, :-1] - rs[:, 1:]) > 1e-3
    return apart & torch.cat([torch.ones(rs.shape[0], 1, dtype=torch.bool), apart[:, :-1]], 1)


def randn_logits(rows, V, seed):
    return (torch.randn(rows, V, generator=torch.Generator().manual_seed(seed)) * 2).to(torch.bfloat16)


@pytest.fixture(scope="module")
def tiny(gpu):
    return _model("tiny", gpu)


@pytest.mark.parametrize("n_hist", [1, 7, 70, 500])
@pytest.mark.parametrize("p", [1.8, 0.6])
@pytest.mark.parametrize("V", [256, 262144])
def test_beam_candidates_greedy_penalised_vs_hf(gpu, tiny, V, p, n_hist):
    """do_sample=False, B 2 x K 3, 6 candidates: n_hist 70 takes the kept list beyond one wave, 500 + 6 is close to
    the capacity.  Scores within the bar, (token, beam) equal at every pinned place, at least 1/3 of the places
    pinned, and HF's candidates with the penalty differ from those without (a no-op implementation fails)."""
    _, _, lm = tiny
    B, K, NC = 2, 3, 6
    lg = randn_logits(B * K, V, 3)
    bs = torch.tensor(BEAM_SCORES * B)
    hist = history(lg, n_hist, 5)
    rt, rb, rs, _ = ref_beam_candidates(lg, bs, K, NC + 1, hist, p)
    ut, ub, _, _ = ref_beam_candidates(lg, bs, K, NC + 1, None, 1.0)
    assert not (torch.equal(rt, ut) and torch.equal(rb, ub)), "the penalty does not change the reference"
    tok, bi, sc = lm.beam_candidates(lg.to(gpu), bs, K, NC, False, 0, 1.0, 1.0, 0, 0, 1, history=hist.to(gpu),
                                     repetition_penalty=p)
    print("max |score - ref|", float((sc.cpu() - rs[:, :-1]).abs().max()))
    torch.testing.assert_close(sc.cpu(), rs[:, :-1], rtol=0, atol=2e-4 * max(1.0, p))
    pinned = pinned_places(rs)
    same = (tok.cpu() == rt[:, :-1]) & (bi.cpu().long() == rb[:, :-1])
    assert pinned.float().mean() >= 1 / 3, pinned
    assert bool(same[pinned].all()), (tok, rt, bi, rb)


def test_beam_candidates_sampling_penalised_law(gpu, tiny):
    """do_sample (T 0.8, top_k 50, top_p 0.9, min_tokens_to_keep 2, 2 beams, 4 draws, p 1.8, 7 history tokens):
    every draw in HF's processed support, no (beam, token) twice in an item, scores within the bar, the first draw
    distributed as softmax(accumulated) (TV within 3x its expectation over 4096 items), the seed repeats the
    draws; the support differs from the unpenalised one."""
    cfg, _, lm = tiny
    K, V, N, p = 2, cfg.vocab_size, 4096, 1.8
    one = randn_logits(K, V, 9)
    hist1 = history(one, 7, 6)
    lg = one.repeat(N, 1).to(gpu)
    hist = hist1.repeat(N, 1).to(gpu)
    bs = torch.tensor([0.0, -0.5]).repeat(N)
    kw = dict(do_sample=True, top_k=50, top_p=0.9, temperature=0.8, min_keep=2)
    acc = ref_beam_candidates(one, bs[:K], K, 4, hist1, p, **kw)[3][0]
    acc0 = ref_beam_candidates(one, bs[:K], K, 4, None, 1.0, **kw)[3][0]
    assert not torch.equal(torch.isfinite(acc), torch.isfinite(acc0)), "the penalty does not change the support"
    run = lambda seed: lm.beam_candidates(lg, bs, K, 4, True, 50, 0.9, 0.8, seed, 0, 2, history=hist,
                                          repetition_penalty=p)
    tok, bi, sc = run(11)
    tok, bi = tok.cpu(), bi.cpu().long()
    flat = bi * V + tok
    assert (tok >= 0).all()
    assert torch.isfinite(acc[flat]).all(), "a draw outside the processed support"
    assert all(len(set(row.tolist())) == 4 for row in flat[:64]), "drawn twice"
    torch.testing.assert_close(sc.cpu(), acc[flat], rtol=0, atol=2e-4 * p)
    pr = torch.softmax(acc.double(), -1)
    emp = torch.bincount(flat[:, 0], minlength=K * V).double() / N
    tv = 0.5 * float((emp - pr).abs().sum())
    bar = 3.0 * 0.5 * float((2.0 * pr * (1 - pr) / (np.pi * N)).sqrt().sum())
    print("tv", tv, "bar", bar)
    assert tv < bar, (tv, bar)
    assert torch.equal(run(11)[0].cpu(), tok) and not torch.equal(run(12)[0].cpu(), tok)


def ref_sample_row(lg, hist, p, do_sample=False, top_k=0, top_p=1.0, temperature=1.0):
    """_sample's processed row: the penalty on the raw fp32 logits, then the warpers (as log probs; -inf = dropped)."""
    from oracle import beam_ref as BR
    pen = hf_penalise(hist, lg.float(), p)
    return BR.processed_log_probs(pen, True, top_k, top_p, temperature, 1) if do_sample else pen


@pytest.mark.parametrize("p", [1.8, 0.6])
@pytest.mark.parametrize("V", [256, 262144])
def test_sample_next_token_greedy_penalised_vs_hf(gpu, V, p):
    """Greedy = the argmax of HF's penalised fp32 row wherever its top two are more than 1e-3 apart (V 256: distinct
    logits, so every row is pinned).  The history holds the row's top-4 -- positive logits, divided -- and its
    bottom-2 -- negative, multiplied: with p 0.6 a divided one stays or becomes the argmax, with 1.8 they leave."""
    from projectiontrainer_amd import kernels as KK
    B = 8
    lg = _distinct_logits(B, V, 3) if V == 256 else randn_logits(B, V, 4)
    for n_hist in (7, 70):
        hist = history(lg, n_hist, 8)
        hist[:, 4:6] = (-lg.float()).topk(2, -1).indices
        assert bool((torch.gather(lg.float(), 1, hist[:, :4]) > 0).all())
        assert bool((torch.gather(lg.float(), 1, hist[:, 4:6]) < 0).all())
        ref = ref_sample_row(lg, hist, p)
        top2 = ref.topk(2, -1)
        pinned = (top2.values[:, 0] - top2.values[:, 1]) > 1e-3
        assert pinned.float().mean() >= 1 / 3 and (V > 256 or bool(pinned.all()))
        if p > 1:
            assert not torch.equal(top2.indices[:, 0], lg.float().argmax(-1)), "the penalty does not move the argmax"
        got = KK.sample_next_token(lg.to(gpu), history=hist.to(gpu), repetition_penalty=p).cpu()
        assert torch.equal(got[pinned], top2.indices[:, 0][pinned]), (got, top2.indices[:, 0])
    # a negative maximum is multiplied: a row of negative logits whose maximum is in the history
    neg = (lg.float() - (8.0 if V == 256 else 20.0)).to(torch.bfloat16)   # (V 256: still distinct, -16 .. -1/16)
    assert bool((neg.float() < 0).all())
    hist = neg.float().topk(1, -1).indices
    ref = ref_sample_row(neg, hist, p)
    top2 = ref.topk(2, -1)
    pinned = (top2.values[:, 0] - top2.values[:, 1]) > 1e-3
    got = KK.sample_next_token(neg.to(gpu), history=hist.to(gpu), repetition_penalty=p).cpu()
    assert bool(pinned.any()) and torch.equal(got[pinned], top2.indices[:, 0][pinned])


@pytest.mark.parametrize("V", [512, 262144])
def test_sample_next_token_sampling_penalised_law(gpu, V):
    """4096 rows of one logits row (T 0.8, top_k 50, top_p 0.9, p 1.8, 7 history tokens): every draw in HF's
    processed support, distributed as its softmax (TV within 3x its expectation); the seed repeats the draws."""
    from projectiontrainer_amd import kernels as KK
    N, p = 4096, 1.8
    one = randn_logits(1, V, 13 if V == 512 else 18)
    hist1 = history(one, 7, 14)
    kw = dict(do_sample=True, top_k=50, top_p=0.9, temperature=0.8)
    ref = ref_sample_row(one, hist1, p, **kw)[0]
    # the top-p cut must not fall between equal values: there HF's (unstable) sort picks the survivors
    pen = hf_penalise(hist1, one.float(), p)[0]
    cut = (pen >= pen.topk(50).values[-1]) & ~torch.isfinite(ref)
    assert not bool(cut.any()) or float(pen[cut].max()) < float(pen[torch.isfinite(ref)].min())
    ref0 = ref_sample_row(one, None, 1.0, **kw)[0]
    assert not torch.equal(torch.isfinite(ref), torch.isfinite(ref0)), "the penalty does not change the support"
    lg, hist = one.repeat(N, 1).to(gpu), hist1.repeat(N, 1).to(gpu)
    run = lambda seed: KK.sample_next_token(lg, history=hist, repetition_penalty=p, seed=seed, step=3, **kw).cpu()
    tok = run(21)
    assert torch.isfinite(ref[tok]).all(), "a draw outside the processed support"
    pr = torch.softmax(ref.double(), -1)
    emp = torch.bincount(tok, minlength=V).double() / N
    tv = 0.5 * float((emp - pr).abs().sum())
    bar = 3.0 * 0.5 * float((2.0 * pr * (1 - pr) / (np.pi * N)).sqrt().sum())
    print("tv", tv, "bar", bar)
    assert tv < bar, (tv, bar)
    assert torch.equal(run(21), tok) and not torch.equal(run(22), tok)


def test_penalty_off_is_the_unpenalised_path(gpu, tiny):
    """p = 1 with a history, and p = 1.8 with an empty one, equal the unpenalised entry points exactly: the three
    outputs of ptk_beam_candidates (greedy and sampled), the sampled token, and generate's tokens and logits."""
    from projectiontrainer_amd import kernels as KK
    cfg, _, lm = tiny
    B, K, V = 2, 3, cfg.vocab_size
    lg = randn_logits(B * K, V, 17).to(gpu)
    bs = torch.tensor(BEAM_SCORES * B)
    hist = history(lg.cpu(), 7, 18).to(gpu)
    empty = hist[:, :0].contiguous()
    for args in ((False, 0, 1.0, 1.0, 0, 0, 1), (True, 50, 0.9, 0.8, 5, 2, 2)):
        base = lm.beam_candidates(lg, bs, K, 6, *args)
        for h, p in ((hist, 1.0), (empty, 1.8), (None, 1.8)):
            got = lm.beam_candidates(lg, bs, K, 6, *args, history=h, repetition_penalty=p)
            assert all(torch.equal(a, b) for a, b in zip(base, got)), (args, p)
    kw = dict(do_sample=True, top_k=50, top_p=0.9, temperature=0.8, seed=3, step=1)
    base = KK.sample_next_token(lg, **kw)
    assert torch.equal(base, KK.sample_next_token(lg, history=hist, repetition_penalty=1.0, **kw))
    assert torch.equal(base, KK.sample_next_token(lg, history=empty, repetition_penalty=1.8, **kw))
    x = torch.randn(3, 12, cfg.hidden_size, generator=torch.Generator().manual_seed(19)).to(gpu)
    g = dict(max_new_tokens=8, do_sample=True, top_k=50, top_p=0.9, temperature=0.8, seed=4, return_logits=True)
    t0, l0 = lm.generate(x, **g)
    t1, l1 = lm.generate(x, repetition_penalty=1.0, **g)
    assert torch.equal(t0, t1) and torch.equal(l0, l1)
    # one new token has no history yet: p = 1.8 is the unpenalised call as well
    g1 = dict(g, max_new_tokens=1)
    a, b = lm.generate(x, **g1), lm.generate(x, repetition_penalty=1.8, **g1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_penalised_entry_points_with_penalty_off_are_the_plain_ones(gpu, tiny):
    """The C entry points themselves (the Python methods pick the plain ones when the penalty is off, so they do not
    reach this): ptk_beam_candidates_penalized with (history, p = 1) and (n_hist = 0, p = 1.8), greedy and sampled,
    writes the three outputs of ptk_beam_candidates bit for bit, into the plain call's workspace size; and
    ptk_gemma3_generate_penalized with p = 1 gives ptk_gemma3_generate's tokens and step_logits."""
    from projectiontrainer_amd import _lib as L
    cfg, _, lm = tiny
    lib, st = L.lib(), L.stream_ptr(gpu)
    B, K, NC, V = 2, 3, 6, cfg.vocab_size
    lg = randn_logits(B * K, V, 41).to(gpu)
    bs = torch.tensor(BEAM_SCORES * B, device=gpu)
    hist = history(lg.cpu(), 7, 42).to(gpu)
    n_ws = lib.ptk_beam_candidates_workspace_bytes(B, K, NC)

    def outputs():
        return (torch.full((B, NC), -7, dtype=torch.int64, device=gpu),
                torch.full((B, NC), -7, dtype=torch.int32, device=gpu),
                torch.full((B, NC), -7.0, dtype=torch.float32, device=gpu),
                torch.zeros(n_ws, dtype=torch.uint8, device=gpu))
    for do_sample, top_k, top_p, T, seed, step, keep in ((0, 0, 1.0, 1.0, 0, 0, 1), (1, 50, 0.9, 0.8, 5, 2, 2)):
        t0, b0, s0, w0 = outputs()
        L.check(lib.ptk_beam_candidates(lg.data_ptr(), V, bs.data_ptr(), B, K, V, do_sample, top_k, top_p, T, keep,
                                        seed, step, NC, t0.data_ptr(), b0.data_ptr(), s0.data_ptr(), w0.data_ptr(),
                                        n_ws, st), "ptk_beam_candidates")
        assert bool((t0 >= 0).all())
        for h, ld, n_hist, p in ((hist.data_ptr(), 7, 7, 1.0), (hist.data_ptr(), 7, 0, 1.8), (None, 0, 0, 1.8)):
            t1, b1, s1, w1 = outputs()
            L.check(lib.ptk_beam_candidates_penalized(lg.data_ptr(), V, bs.data_ptr(), B, K, V, do_sample, top_k, top_p,
                                                      T, keep, seed, step, NC, h, ld, n_hist, p, t1.data_ptr(),
                                                      b1.data_ptr(), s1.data_ptr(), w1.data_ptr(), n_ws, st),
                    "ptk_beam_candidates_penalized")
            assert torch.equal(t0, t1) and torch.equal(b0, b1) and torch.equal(s0, s1), (do_sample, n_hist, p)
            assert torch.equal(w0, w1)   # the same scratch contents: the same kernels wrote them
    Bg, P, NT = 3, 12, 8
    x = torch.randn(Bg, P, cfg.hidden_size, generator=torch.Generator().manual_seed(43)).to(gpu)
    n_gen = lib.ptk_gemma3_generate_workspace_bytes(lm.c_cfg, Bg, P, NT)
    for do_sample in (0, 1):
        desc = L.Gemma3GenerateC(Bg, P, NT, do_sample, 50, 0.8, 4, -1, 0, P, 0.9)
        res = []
        for penalised in (False, True):
            ws = torch.zeros(n_gen, dtype=torch.uint8, device=gpu)
            out = torch.full((Bg, NT), -7, dtype=torch.int64, device=gpu)
            logits = torch.zeros((NT, Bg, V), dtype=torch.bfloat16, device=gpu)
            head = (lm.c_cfg, lm.c_w, desc, x.data_ptr(), None, out.data_ptr(), logits.data_ptr())
            if penalised:
                L.check(lib.ptk_gemma3_generate_penalized(*head, 1.0, ws.data_ptr(), n_gen, st), "generate_penalized")
            else:
                L.check(lib.ptk_gemma3_generate(*head, ws.data_ptr(), n_gen, st), "generate")
            res.append((out, logits))
        assert bool((res[0][0] >= 0).all())
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), do_sample


def test_generate_penalised_teacher_forced_vs_hf(gpu, tiny):
    """tiny (V 512), B 3, 12 steps.  Run A: greedy, p 1 -> tokens a and every step's logits.  Run B: teacher-forced
    with a, p 1.8: the same logits bit for bit (step_logits are the raw ones), and the token of step t is the
    argmax of HF's processor over (a[:, :t], fp32(logits[t])) wherever that row's top two are > 1e-3 apart."""
    cfg, _, lm = tiny
    B, NT, p = 3, 12, 1.8
    x = torch.randn(B, 12, cfg.hidden_size, generator=torch.Generator().manual_seed(23)).to(gpu)
    a, la = lm.generate(x, max_new_tokens=NT, do_sample=False, return_logits=True)
    b, lb = lm.generate(x, max_new_tokens=NT, do_sample=False, return_logits=True, force_ids=a,
                        repetition_penalty=p)
    assert torch.equal(la, lb)
    a, b, la = a.cpu(), b.cpu(), la.float().cpu()
    pinned_n = total = 0
    for t in range(NT):
        ref = hf_penalise(a[:, :t], la[t], p)
        top2 = ref.topk(2, -1)
        pinned = (top2.values[:, 0] - top2.values[:, 1]) > 1e-3
        assert torch.equal(b[:, t][pinned], top2.indices[:, 0][pinned]), (t, b[:, t], top2.indices[:, 0])
        pinned_n += int(pinned.sum())
        total += B
    assert pinned_n / total >= 1 / 3
    assert not torch.equal(a, b), "the penalty never changed a token"


def test_beam_generate_penalised_end_to_end(gpu, tiny):
    """beam_generate(repetition_penalty=1.8, do_sample=False): two runs identical, the shape rules of
    test_beam_generate_end_to_end, and a result that differs from p = 1."""
    cfg, _, lm = tiny
    x = torch.randn(3, 20, cfg.hidden_size, generator=torch.Generator().manual_seed(5)).to(gpu)
    mask = torch.ones(3, 20, dtype=torch.long)
    mask[1, 16:18] = 0
    kw = dict(num_beams=3, max_new_tokens=10, do_sample=False)
    a = lm.beam_generate(x, mask.to(gpu), repetition_penalty=1.8, **kw)
    b = lm.beam_generate(x, mask.to(gpu), repetition_penalty=1.8, **kw)
    base = lm.beam_generate(x, mask.to(gpu), **kw)
    assert torch.equal(a, b) and a.shape == (3, 10)
    assert not torch.equal(a, base)
    eos = int(a[0, 2])
    c = lm.beam_generate(x, mask.to(gpu), repetition_penalty=1.8, eos_token_id=eos, pad_token_id=0, **kw).cpu()
    assert c.shape[0] == 3 and c.shape[1] <= 10
    for row in c:
        hit = (row == eos).nonzero()
        if hit.numel():
            assert (row[int(hit[0]) + 1:] == eos).all()


def test_beam_generate_history_is_the_running_hypothesis(gpu, tiny):
    """beam_generate keeps each row's history on the device; the same search written out with the history taken
    from the host bookkeeping, BeamSearch.run_seq[:, :, :t] (the row's hypothesis after the beam re-order), gives
    the same tokens, greedy and sampled."""
    from projectiontrainer_amd.beam import BeamSearch
    cfg, _, lm = tiny
    B, K, NT, p = 3, 3, 10, 1.8
    x = torch.randn(B, 20, cfg.hidden_size, generator=torch.Generator().manual_seed(5)).to(gpu)
    mask = torch.ones(B, 20, dtype=torch.long)
    mask[1, 16:18] = 0
    for kw in (dict(do_sample=False, top_k=0, top_p=1.0, temperature=1.0),
               dict(do_sample=True, top_k=50, top_p=0.9, temperature=0.8)):
        got = lm.beam_generate(x, mask.to(gpu), num_beams=K, max_new_tokens=NT, repetition_penalty=p, seed=3, **kw)
        bs = BeamSearch(B, K, NT, None, cfg.pad_token_id, 1.0, False)
        logits = lm.decode_begin(x, mask.to(gpu), repeat=K, max_new_tokens=NT)
        step = 0
        while True:
            hist = bs.run_seq[:, :, :step].reshape(B * K, step) if step else None
            tok, bi, sc = lm.beam_candidates(logits, bs.run_score.reshape(-1), K, 2 * K, kw["do_sample"], kw["top_k"],
                                             kw["top_p"], kw["temperature"], 3, step, 1, history=hist,
                                             repetition_penalty=p)
            ids, rows = bs.step(tok, bi, sc)
            if bs.finished:
                break
            step += 1
            logits = lm.decode_next(step, ids, rows)
        assert torch.equal(got.cpu(), bs.result()), kw


def test_over_capacity_is_an_error_before_any_launch(gpu, tiny):
    """top-k + history above the 1024 entries of the LDS lists: the call fails and ptk_last_error names the limit
    (the check is on the host, ahead of the launch: tests/test_repetition_penalty_host.py runs it on host memory);
    at the limit the call runs."""
    from projectiontrainer_amd import _lib as L
    from projectiontrainer_amd import kernels as KK
    cfg, _, lm = tiny
    V = cfg.vocab_size
    lg = randn_logits(3, V, 29).to(gpu)
    hist = torch.zeros(3, 1000, dtype=torch.int64, device=gpu)
    with pytest.raises(L.PtkError, match="1024"):
        KK.sample_next_token(lg, do_sample=True, top_k=50, history=hist, repetition_penalty=1.8)
    with pytest.raises(L.PtkError, match="1024"):
        lm.beam_candidates(lg, torch.tensor(BEAM_SCORES), 3, 6, True, 50, 0.9, 0.8, 0, 0, 2, history=hist,
                           repetition_penalty=1.8)
    with pytest.raises(L.PtkError, match="1024"):
        lm.beam_candidates(lg, torch.tensor(BEAM_SCORES), 3, 6, False, 0, 1.0, 1.0, 0, 0, 1,
                           history=torch.zeros(3, 1019, dtype=torch.int64, device=gpu), repetition_penalty=1.8)
    x = torch.randn(1, 8, cfg.hidden_size, generator=torch.Generator().manual_seed(31)).to(gpu)
    with pytest.raises(L.PtkError, match="1024"):
        lm.generate(x, max_new_tokens=1000, do_sample=True, top_k=50, repetition_penalty=1.8)
    # within the limit the same calls run: 974 + 50 = 1024
    ok = KK.sample_next_token(lg, do_sample=True, top_k=50, history=hist[:, :974].contiguous(), repetition_penalty=1.8)
    assert ok.shape == (3,) and bool(((ok >= 0) & (ok < V)).all())


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf"), "1.8"])
def test_python_rejects_invalid_penalty(gpu, tiny, bad):
    from projectiontrainer_amd import _lib as L
    cfg, _, lm = tiny
    x = torch.randn(1, 8, cfg.hidden_size, generator=torch.Generator().manual_seed(37)).to(gpu)
    with pytest.raises(L.PtkError, match="repetition_penalty"):
        lm.generate(x, max_new_tokens=2, repetition_penalty=bad)
    with pytest.raises(L.PtkError, match="repetition_penalty"):
        lm.beam_generate(x, None, num_beams=2, max_new_tokens=2, repetition_penalty=bad)


def test_python_accepts_any_real_scalar_penalty(gpu, tiny):
    cfg, _, lm = tiny
    x = torch.randn(1, 8, cfg.hidden_size, generator=torch.Generator().manual_seed(37)).to(gpu)
    base = lm.generate(x, max_new_tokens=3, do_sample=False, repetition_penalty=1.8)
    for p in (np.float32(1.8), torch.tensor(1.8), np.float64(1.8)):
        assert torch.equal(base, lm.generate(x, max_new_tokens=3, do_sample=False, repetition_penalty=p))
