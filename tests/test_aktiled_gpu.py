"""k-step-tiled activations on the GPU, bit for bit (torch.equal) against the row-major launches: the 8-wave kernel
reading a tiled A (ptk_gemm_desc.A_kt), the 4-wave kernel's GEGLU and GEGLU-backward epilogues writing tiled outputs
(C_kt, aux_kt) and reading tiled factors (aux_in_kt), the refusals, the two producer -> consumer chains of the Gemma
MLP, and one Stage-1 step with PTK_A_KTILED 1 and 0.

The flags say how the operand's own buffer is laid out (there is no second pointer as for B_kt), so the proof that a
launch read or wrote the tiled order is the layout itself: a tiled buffer read as row-major is another matrix (a
permutation of random values), and the outputs are compared after un-tiling with tests/ktiled_util.py's index.  Every
tiled output buffer is longer than the matrix (M rounded up to 256 rows) and prefilled with a sentinel, which must
survive past byte M * width * 2."""
import functools

import numpy as np
import pytest
import torch

from tests.ktiled_util import tiled_source_index

pytestmark = pytest.mark.gpu
SENT = 0x7B5A   # bf16 bit pattern of the sentinel


def _k():
    from projectiontrainer_amd import kernels as Kn, _lib as L
    return Kn, L


def rnd(*shape, dev, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).to(dev)


def sentinel(rows, cols, dev):
    return torch.full((rows, cols), SENT, dtype=torch.int16, device=dev).view(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _index(M, W):
    return tiled_source_index(M, W)


def untile(buf, M, W):
    """Row-major [M, W] of the tiled form held by the first M * W elements of buf."""
    idx = torch.from_numpy(_index(M, W)).to(buf.device)
    out = torch.empty(M * W, dtype=torch.int16, device=buf.device)
    out[idx] = buf.reshape(-1)[:M * W].view(torch.int16)
    return out.view(M, W).view(torch.bfloat16)


def tail_is_sentinel(buf, M, W):
    return bool((buf.reshape(-1)[M * W:].view(torch.int16) == SENT).all())


def _forced(L, mode, fn):
    """fn() under force mode `mode`: its result, the kernel families it ran and the tiled-launch counters."""
    L.lib().ptk_gemm_force_small_tiles(mode)
    L.gemm_path_counts(reset=True)
    L.gemm_ktiled_counts(reset=True)
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, {p for p, _ in L.gemm_path_counts(reset=True)}, L.gemm_ktiled_counts(reset=True)
    finally:
        L.lib().ptk_gemm_force_small_tiles(0)


# ------------------------------------------------------------------ consumer: the 8-wave kernel reading a tiled A
def _check_consumer(gpu, mode, M, N, K):
    Kn, L = _k()
    A, B = rnd(M, K, dev=gpu, seed=61), rnd(N, K, dev=gpu, seed=62, scale=0.05)
    Bkt, Akt = Kn.pack_kstep_tiles(B), Kn.pack_kstep_tiles(A)
    ref, p0, c0 = _forced(L, mode, lambda: Kn.gemm(A, B, B_kt=Bkt))
    got, p1, c1 = _forced(L, mode, lambda: Kn.gemm(Akt, B, B_kt=Bkt, A_kt=True))
    assert p0 == p1 == {"p8"}, (p0, p1)
    assert c0 == (0, 0) and c1 == (1, 0), (c0, c1)
    assert torch.equal(ref, got), (ref.float() - got.float()).abs().max()
    return A, B, Bkt, ref


@pytest.mark.parametrize("K", [128, 1152])
@pytest.mark.parametrize("mode", [32, 512, 1024, 4096])   # 256-, 224-, 192- and 160-row tiles
def test_p8_reads_tiled_a(gpu, mode, K):
    """M 320: a ragged second row tile with 4 real 16-row groups (at every tile height), the others past the end."""
    _check_consumer(gpu, mode, 320, 272, K)


def test_row_major_anchor_is_the_gemm(gpu):
    """The row-major launch the tiled ones are compared with is A . B^T (so "equal" is not two empty outputs)."""
    Kn, L = _k()
    A, B, Bkt, ref = _check_consumer(gpu, 32, 320, 272, 1152)
    f32, _, _ = _forced(L, 32, lambda: Kn.gemm(A, B, out_dtype=torch.float32, B_kt=Bkt))
    plain = A.float() @ B.float().T
    torch.testing.assert_close(f32, plain, rtol=2e-3, atol=2e-3 * 1152 ** 0.5)
    torch.testing.assert_close(ref.float(), plain, rtol=2e-2, atol=2e-2)   # (test_ktiled_gpu's bf16 bound)


def test_tiled_a_stream_crosses_tile_boundaries(gpu):
    """Two full rounds of the persistent grid plus one tile (3 column tiles): every workgroup's A stream runs out of
    one tile into the next with the tiled offsets; the last row tile is ragged (160 real rows)."""
    ncu = torch.cuda.get_device_properties(gpu).multi_processor_count
    nbm = (2 * ncu + 1 + 2) // 3
    _check_consumer(gpu, 32, nbm * 256 - 96, 528, 128)


# ------------------------------------------------------------------ producers: the 4-wave kernel's tiled epilogues
@pytest.mark.parametrize("factors", [True, False])
@pytest.mark.parametrize("K", [64, 1152])
def test_geglu_writes_tiled_outputs(gpu, K, factors):
    """M 320, N 320: h, a, b are 160 columns = 5 k-steps, the second column tile holds one real k-step."""
    Kn, L = _k()
    M, N, Mp = 320, 320, 512
    W = N // 2
    A, B = rnd(M, K, dev=gpu, seed=71), rnd(N, K, dev=gpu, seed=72, scale=0.05)
    Bkt = Kn.pack_kstep_tiles(B)
    r = [sentinel(Mp, W, gpu) for _ in range(3)]
    t = [sentinel(Mp, W, gpu) for _ in range(3)]
    _, p0, c0 = _forced(L, 8, lambda: Kn.gemm(A, B, act=L.ACT_GEGLU, C=r[0][:M], aux=r[1][:M], aux2=r[2][:M], B_kt=Bkt))
    _, p1, c1 = _forced(L, 8, lambda: Kn.gemm(A, B, act=L.ACT_GEGLU, C=t[0], aux=t[1], aux2=t[2], B_kt=Bkt,
                                              C_kt=True, aux_kt=factors))
    assert p0 == p1 == {"w4"} and c0 == (0, 0) and c1 == (0, 1), (p0, p1, c0, c1)
    assert r[0][:M].view(torch.int16).ne(SENT).any()
    for i in range(3):
        tiled = i == 0 or factors
        got = untile(t[i], M, W) if tiled else t[i][:M]
        assert torch.equal(got, r[i][:M]), i
        assert tail_is_sentinel(t[i], M, W) and tail_is_sentinel(r[i], M, W), i


@pytest.mark.parametrize("factors", [True, False])
@pytest.mark.parametrize("K", [64, 1152])
def test_geglu_bwd_writes_tiled_output_and_reads_tiled_factors(gpu, K, factors):
    """M 320, N 288: dg | du is 576 columns = 18 k-steps; the second column tile holds one real k-step of dh (two of
    dg | du), the column pairs after it are skipped."""
    Kn, L = _k()
    M, N, Mp = 320, 288, 512
    A, B = rnd(M, K, dev=gpu, seed=73), rnd(N, K, dev=gpu, seed=74, scale=0.05)
    Bkt = Kn.pack_kstep_tiles(B)
    a, b = rnd(M, N, dev=gpu, seed=75), rnd(M, N, dev=gpu, seed=76)
    ain, bin_ = (Kn.pack_kstep_tiles(a), Kn.pack_kstep_tiles(b)) if factors else (a, b)
    r, t = sentinel(Mp, 2 * N, gpu), sentinel(Mp, 2 * N, gpu)
    _, p0, c0 = _forced(L, 8, lambda: Kn.gemm(A, B, act=L.ACT_GEGLU_BWD, C=r[:M], aux_in=a, aux_in2=b, B_kt=Bkt))
    _, p1, c1 = _forced(L, 8, lambda: Kn.gemm(A, B, act=L.ACT_GEGLU_BWD, C=t, aux_in=ain, aux_in2=bin_, B_kt=Bkt,
                                              C_kt=True, aux_in_kt=factors))
    assert p0 == p1 == {"w4"} and c0 == (0, 0) and c1 == (0, 1), (p0, p1, c0, c1)
    assert r[:M].view(torch.int16).ne(SENT).all()
    assert torch.equal(untile(t, M, 2 * N), r[:M])
    assert tail_is_sentinel(t, M, 2 * N) and tail_is_sentinel(r, M, 2 * N)


# ------------------------------------------------------------------ refusals
def test_tiled_c_refused_when_m_is_not_whole_groups(gpu):
    Kn, L = _k()
    M, N, K = 328, 320, 64
    A, B = rnd(M, K, dev=gpu, seed=81), rnd(N, K, dev=gpu, seed=82, scale=0.05)
    Bkt, C = Kn.pack_kstep_tiles(B), sentinel(512, N // 2, gpu)
    g, u = sentinel(512, N // 2, gpu), sentinel(512, N // 2, gpu)
    L.lib().ptk_gemm_force_small_tiles(8)
    try:
        with pytest.raises(L.PtkError, match="k-step-tiled"):
            Kn.gemm(A, B, act=L.ACT_GEGLU, C=C, aux=g, aux2=u, B_kt=Bkt, C_kt=True, aux_kt=True)
    finally:
        L.lib().ptk_gemm_force_small_tiles(0)
    torch.cuda.synchronize()
    assert all(tail_is_sentinel(x, 0, N // 2) for x in (C, g, u))
    assert L.gemm_ktiled_counts(reset=True) == (0, 0)


def test_tiled_a_refused_by_sliced_batched_and_other_family_launches(gpu):
    """A K-sliced launch is a batch of slices over a part of each row of A (what gemm_split makes): refused with a
    tiled A, as are a family without the variant (the 4-wave kernel), an fp32 output and a missing tiled B."""
    Kn, L = _k()
    M, N, K = 320, 272, 256
    A, B = rnd(M, K, dev=gpu, seed=83), rnd(N, K, dev=gpu, seed=84, scale=0.05)
    Akt, Bkt = Kn.pack_kstep_tiles(A), Kn.pack_kstep_tiles(B)
    part = sentinel(2 * M, 2 * N, gpu).view(torch.float32)
    cases = [
        (32, dict(C=part, K=K // 2, batch=2, strides=(K // 2, 0, K // 2, 0, M * N, 0), lda=K, ldb=K, B_kt=Bkt)),
        (8, dict(B_kt=Bkt)),
        (32, dict(B_kt=Bkt, out_dtype=torch.float32)),
        (32, dict()),
    ]
    for mode, kw in cases:
        L.lib().ptk_gemm_force_small_tiles(mode)
        try:
            with pytest.raises(L.PtkError, match="k-step-tiled"):
                Kn.gemm(Akt, B, A_kt=True, **kw)
        finally:
            L.lib().ptk_gemm_force_small_tiles(0)
    torch.cuda.synchronize()
    assert bool((part.view(torch.int16) == SENT).all())
    assert L.gemm_ktiled_counts(reset=True) == (0, 0)


# ------------------------------------------------------------------ the two chains of the Gemma MLP
@pytest.mark.parametrize("factors", [True, False])
def test_mlp_chains_tiled_against_row_major(gpu, factors):
    """gate|up (tiled h, a, b) -> down (tiled A) and dh (tiled a, b in, tiled dg | du out) -> d(gate|up) dX at M 512,
    hidden 128, intermediate 256; producers forced onto the 4-wave kernel, consumers onto the 8-wave one."""
    Kn, L = _k()
    M, H, I = 512, 128, 256
    x, dd = rnd(M, H, dev=gpu, seed=91), rnd(M, H, dev=gpu, seed=92)
    wgu, wd = rnd(2 * I, H, dev=gpu, seed=93, scale=0.05), rnd(H, I, dev=gpu, seed=94, scale=0.05)
    wd_t, wgu_t = wd.t().contiguous(), wgu.t().contiguous()
    kt = {k: Kn.pack_kstep_tiles(v) for k, v in dict(wgu=wgu, wd=wd, wd_t=wd_t, wgu_t=wgu_t).items()}

    def chain(tiled):
        fac = tiled and factors
        h, a, b = (torch.empty(M, I, dtype=torch.bfloat16, device=gpu) for _ in range(3))
        dgu = torch.empty(M, 2 * I, dtype=torch.bfloat16, device=gpu)
        fams, cnt = [], []

        def run(mode, fn):
            out, p, c = _forced(L, mode, fn)
            fams.append(p)
            cnt.append(c)
            return out

        run(8, lambda: Kn.gemm(x, wgu, act=L.ACT_GEGLU, C=h, aux=a, aux2=b, B_kt=kt["wgu"], C_kt=tiled, aux_kt=fac))
        dn = run(32, lambda: Kn.gemm(h, wd, B_kt=kt["wd"], A_kt=tiled))
        run(8, lambda: Kn.gemm(dd, wd_t, act=L.ACT_GEGLU_BWD, C=dgu, aux_in=a, aux_in2=b, B_kt=kt["wd_t"], C_kt=tiled,
                               aux_in_kt=fac))
        dx = run(32, lambda: Kn.gemm(dgu, wgu_t, B_kt=kt["wgu_t"], A_kt=tiled))
        assert fams == [{"w4"}, {"p8"}, {"w4"}, {"p8"}], fams
        assert cnt == ([(0, 1), (1, 0)] * 2 if tiled else [(0, 0)] * 4), cnt
        return dn, dx, h, dgu

    ref, got = chain(False), chain(True)
    assert torch.equal(ref[0], got[0]) and torch.equal(ref[1], got[1])
    assert torch.equal(ref[2], untile(got[2], M, I)) and torch.equal(ref[3], untile(got[3], M, 2 * I))
    assert ref[0].float().abs().max() > 0 and ref[1].float().abs().max() > 0


# ------------------------------------------------------------------ the model
def _stage1_cfg():
    from projectiontrainer_amd.config import SIGLIP_TINY, Gemma3TextConfig, Stage1Config
    text = Gemma3TextConfig(vocab_size=512, hidden_size=1152, intermediate_size=6912, num_hidden_layers=2,
                            num_attention_heads=4, num_key_value_heads=1, head_dim=256, sliding_window=64,
                            sliding_window_pattern=2, query_pre_attn_scalar=256)
    return Stage1Config(vision=SIGLIP_TINY, text=text, batch_size=MODEL_BATCH, text_len=MODEL_TEXT_LEN)


MODEL_BATCH, MODEL_TEXT_LEN = 16, 240


def test_stage1_step_switch_on_off(gpu, monkeypatch):
    """One Stage-1 step with PTK_A_KTILED 1 and 0 (the switch re-read between them): loss, grad norm and projector
    grads bit-identical; the counters prove the tiled launches ran in one run and not in the other.

    The config is the smallest found on the CPU with ptk_gemm_ktiled_pair / ptk_gemm_split_plan for which the
    predicate says yes on the non-last layer under the default dispatch: Gemma3-1B MLP widths (hidden 1 152,
    intermediate 6 912), 2 layers, vocabulary 512, M = 16 x 256 = 4 096 token rows, the least the persistent kernels
    take (M >= 4 096).  There the down projection (80 tiles, K 6 912) runs unsplit as a single round of the 8-wave
    kernel, so h goes tiled (2 launches: the gate|up write and the down read); d(gate|up) dX (K 13 824, 80 tiles) is
    cut into two K slices by gemm_split, so dg | du and with it the factors stay row-major, which this step checks
    too.  (In the model the backward pair goes tiled only where its 256x256 tiles leave neither a K split nor a lent
    stream-K tail, from about M = 19 712 at these widths, cfg2's 22 528 among them; the chain test above covers it.)"""
    from projectiontrainer_amd import weights as W, _lib as L
    from projectiontrainer_amd.gemma3 import Gemma3CausalLM
    from projectiontrainer_amd.projectors import MLPProjector
    from projectiontrainer_amd.siglip import SiglipVisionTower
    from projectiontrainer_amd.stage1 import Stage1Engine
    cfg = _stage1_cfg()
    M = cfg.batch_size * Gemma3CausalLM.seq_pad(cfg.seq_len)
    assert M == 4096, M
    vp, lp = W.siglip_vision_params(cfg.vision), W.gemma3_params(cfg.text)
    pp = W.projector_params(cfg.vision.hidden_size, cfg.text.hidden_size)
    px, ids, labels = (torch.from_numpy(t).to(gpu) for t in W.synthetic_batch(cfg, seed=5))
    vis = SiglipVisionTower(cfg.vision, vp, gpu)
    llm = Gemma3CausalLM(cfg.text, lp, gpu, max_pos=Gemma3CausalLM.seq_pad(cfg.seq_len))

    def one_step(switch):
        monkeypatch.setenv("PTK_A_KTILED", switch)
        assert L.lib().ptk_a_ktiled_reload() == int(switch)
        proj = MLPProjector(cfg.vision.hidden_size, cfg.text.hidden_size)
        proj.load_state_dict({k: torch.from_numpy(v) for k, v in pp.items()})
        proj.to(gpu)
        eng = Stage1Engine(vis, llm, proj)
        L.gemm_ktiled_counts(reset=True)
        loss = eng.step(px, ids, labels)
        torch.cuda.synchronize()
        return (loss.clone(), eng.grad_norm.clone(), eng.proj.flat_grad.clone()), L.gemm_ktiled_counts(reset=True)

    try:
        on, c_on = one_step("1")
        off, c_off = one_step("0")
    finally:
        monkeypatch.delenv("PTK_A_KTILED")
        L.lib().ptk_a_ktiled_reload()
    assert c_on == (1, 1) and c_off == (0, 0), (c_on, c_off)
    assert torch.isfinite(on[0]).all() and float(on[1]) > 0
    for a, b in zip(on, off):
        assert torch.equal(a, b)


def test_stage2_step_takes_no_tiled_activations(gpu):
    from projectiontrainer_amd import weights as W, _lib as L
    from projectiontrainer_amd.config import PRESETS
    from projectiontrainer_amd.stage2 import synthetic_engine
    cfg = PRESETS["tiny"].replace(batch_size=4, text_len=8 + 12, question_len=8)
    eng = synthetic_engine(cfg, gpu, seed=3, learning_rate=1e-3, total_steps=10)
    px, q, a = (torch.from_numpy(t).to(gpu) for t in W.synthetic_vqa_batch(cfg, seed=9))
    L.gemm_ktiled_counts(reset=True)
    loss = eng.forward_backward(px, q, a)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all()
    assert L.gemm_ktiled_counts(reset=True) == (0, 0)
