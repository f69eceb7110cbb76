"""The persistent GEMMs reading B from its k-step-tiled copy (ptk_gemm_desc.B_kt): the pack kernel against the numpy
statement of the layout, and every kernel family that takes the copy bit for bit (torch.equal) against the same
launch from the row-major B.  The tiled launches get a row-major B of different values (its negation), so a launch
that matches the row-major result has read the tiled copy and nothing else; the launches that must not take the
copy get a copy of different values, so one that matches has read B.

Shapes: M = 320 (a ragged second row tile), N = 272 (the second column tile holds one real 16-row group, the other 15
lie past the buffer and read zero; GEGLU needs N % 32, so N = 288 there: two real groups), K = 64 (one K-tile: the
prologue alone covers the tile; 4-wave kernel only, the 8-wave kernel needs K >= 128), 128 and 1 152; one shape of
two full rounds of the persistent grid plus a tile, so every workgroup's B stream runs from one tile into the next;
a stream-K launch whose plan cuts tiles (a piece starting at k0 != 0)."""
import numpy as np
import pytest
import torch

from tests.ktiled_util import tiled_source_index

pytestmark = pytest.mark.gpu


def _k():
    from projectiontrainer_amd import kernels as Kn, _lib as L
    return Kn, L


def rnd(*shape, dev, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).to(dev)


@pytest.mark.parametrize("N", [16, 48, 272])
@pytest.mark.parametrize("K", [32, 64, 1152])
def test_pack_kernel_matches_numpy_map(gpu, N, K):
    Kn, _ = _k()
    w = rnd(N, K, dev=gpu, seed=N + K)
    got = Kn.pack_kstep_tiles(w).view(torch.int16).cpu().numpy().reshape(-1)
    want = w.view(torch.int16).cpu().numpy().reshape(-1)[tiled_source_index(N, K)]
    assert np.array_equal(got, want)


def _forced(L, mode, fn):
    L.lib().ptk_gemm_force_small_tiles(mode)
    L.gemm_path_counts(reset=True)
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, {p for p, _ in L.gemm_path_counts(reset=True)}
    finally:
        L.lib().ptk_gemm_force_small_tiles(0)


def _check_family(gpu, mode, family, M, N, K, act="plain"):
    """Row-major launch vs the launch from the tiled copy (with a negated row-major B beside it), forced family."""
    Kn, L = _k()
    A, B = rnd(M, K, dev=gpu, seed=31), rnd(N, K, dev=gpu, seed=32, scale=0.05)
    Bkt, wrong = Kn.pack_kstep_tiles(B), -B

    def run(Bm, kt):
        if act == "geglu":
            g = torch.zeros(M, N // 2, dtype=torch.bfloat16, device=gpu)
            u = torch.zeros_like(g)
            return [Kn.gemm(A, Bm, act=L.ACT_GEGLU, aux=g, aux2=u, B_kt=kt), g, u]
        if act == "geglu_bwd":
            gin, uin = rnd(M, N, dev=gpu, seed=33), rnd(M, N, dev=gpu, seed=34)
            return [Kn.gemm(A, Bm, act=L.ACT_GEGLU_BWD, aux_in=gin, aux_in2=uin, B_kt=kt)]
        bias = torch.linspace(-1, 1, N, device=gpu)
        return [Kn.gemm(A, Bm, B_kt=kt), Kn.gemm(A, Bm, out_dtype=torch.float32, B_kt=kt),
                Kn.gemm(A, Bm, bias=bias, act=L.ACT_GELU_TANH, B_kt=kt)]

    ref, p0 = _forced(L, mode, lambda: run(B, None))
    got, p1 = _forced(L, mode, lambda: run(wrong, Bkt))
    assert p0 == p1 == {family}, (p0, p1)
    for r, g in zip(ref, got):
        assert torch.equal(r, g), (r.float() - g.float()).abs().max()
    plain = A.float() @ B.float().T
    if act == "plain":   # and the row-major result is the GEMM (so "equal" is not two empty outputs)
        torch.testing.assert_close(ref[1], plain, rtol=2e-3, atol=2e-3 * K ** 0.5)


@pytest.mark.parametrize("K", [64, 1152])
@pytest.mark.parametrize("act,N", [("plain", 272), ("geglu", 288), ("geglu_bwd", 272)])
def test_w4_reads_tiled_b(gpu, act, N, K):
    _check_family(gpu, 8, "w4", 320, N, K, act)


@pytest.mark.parametrize("K", [128, 1152])
@pytest.mark.parametrize("mode", [32, 512, 1024, 4096])   # 256-, 224-, 192- and 160-row tiles
def test_p8_reads_tiled_b(gpu, mode, K):
    _check_family(gpu, mode, "p8", 320, 272, K)


def test_p8_k64_keeps_row_major_family(gpu):
    """K = 64 is below the 8-wave kernel's K >= 128: the forced launch runs another family, which reads B."""
    Kn, L = _k()
    A, B = rnd(320, 64, dev=gpu, seed=35), rnd(272, 64, dev=gpu, seed=36, scale=0.05)
    garbage = Kn.pack_kstep_tiles(-B)
    ref, _ = _forced(L, 32, lambda: Kn.gemm(A, B))
    got, paths = _forced(L, 32, lambda: Kn.gemm(A, B, B_kt=garbage))
    assert "p8" not in paths and torch.equal(ref, got)


@pytest.mark.parametrize("mode,family", [(8, "w4"), (32, "p8")])
def test_stream_crosses_tile_boundaries(gpu, mode, family):
    """Two full rounds of the persistent grid plus one tile (3 column tiles, the last with one real group): every
    workgroup's LDS-DMA stream runs out of one tile into the next with the tiled offsets."""
    ncu = torch.cuda.get_device_properties(gpu).multi_processor_count
    nbm = (2 * ncu + 1 + 2) // 3
    _check_family(gpu, mode, family, nbm * 256 - 100, 528, 128)


def test_stream_k_tail_reads_tiled_b(gpu):
    """The stream-K tail (10 tiles over the whole grid at K = 4 096: pieces of a few K-tile pairs, nearly all
    starting at k0 != 0) from the tiled copy, bit for bit against the same split from row-major B."""
    Kn, L = _k()
    M, N, K = 1088, 272, 4096
    tail = torch.zeros(L.lib().ptk_gemm_tail_scratch_bytes(), dtype=torch.uint8, device=gpu)
    A, B = rnd(M, K, dev=gpu, seed=41), rnd(N, K, dev=gpu, seed=42, scale=0.03)
    d = L.GemmDesc()
    d.M, d.N, d.K, d.act, d.out, d.tail_ws = M, N, K, L.ACT_NONE, L.OUT_BF16, tail.data_ptr()
    assert L.lib().ptk_gemm_tail_split(d) > 10, "the plan does not cut this shape's tiles"
    Bkt = Kn.pack_kstep_tiles(B)
    ref, p0 = _forced(L, 32, lambda: Kn.gemm(A, B, tail_ws=tail))
    got, p1 = _forced(L, 32, lambda: Kn.gemm(A, -B, tail_ws=tail, B_kt=Bkt))
    assert p0 == p1 == {"p8sk"}, (p0, p1)
    assert torch.equal(ref, got)
    torch.testing.assert_close(ref.float(), A.float() @ B.float().T, rtol=2e-2, atol=2e-2)


def test_launches_that_must_not_take_the_copy(gpu):
    """Batch > 1, a B that is not packed (ldb != K) and a non-persistent family read row-major B whatever B_kt holds.
    (K slices are made by the model-level callers: test_k_sliced_frozen_gemms_read_row_major.)"""
    Kn, L = _k()
    M, N, K = 320, 272, 128
    A, B = rnd(2, M, K, dev=gpu, seed=51), rnd(2, N, K, dev=gpu, seed=52, scale=0.05)
    garbage = Kn.pack_kstep_tiles(-B[0])
    for mode in (8, 32):
        kw = dict(M=M, N=N, K=K, batch=2, strides=(M * K, 0, N * K, 0, M * N, 0),
                  C=torch.zeros(2, M, N, dtype=torch.bfloat16, device=gpu))
        ref, _ = _forced(L, mode, lambda: Kn.gemm(A, B, **kw).clone())
        got, _ = _forced(L, mode, lambda: Kn.gemm(A, B, B_kt=garbage, **kw).clone())
        assert torch.equal(ref, got)
        wide = torch.cat([B[0], B[1][:, :64]], dim=1)   # rows of 192 elements: the left 128 columns are B[0]
        ref, p0 = _forced(L, mode, lambda: Kn.gemm(A[0], B[0]))
        got, p1 = _forced(L, mode, lambda: Kn.gemm(A[0], wide, K=K, ldb=192, B_kt=garbage))
        assert p0 == p1 and torch.equal(ref, got)
    ref, _ = _forced(L, 1, lambda: Kn.gemm(A[0], B[0]))
    got, paths = _forced(L, 1, lambda: Kn.gemm(A[0], B[0], B_kt=garbage))
    assert paths == {"nt128"} and torch.equal(ref, got)


def _stage1_step_on_off(gpu, monkeypatch, cfg, mode):
    """One Stage-1 step of cfg with the frozen towers' tiled copies packed and with PTK_B_KTILED=0, under force
    mode `mode`: (loss, grad norm, projector grads) of both runs."""
    from projectiontrainer_amd import weights as W, _lib as L
    from projectiontrainer_amd.gemma3 import Gemma3CausalLM
    from projectiontrainer_amd.projectors import MLPProjector
    from projectiontrainer_amd.siglip import SiglipVisionTower
    from projectiontrainer_amd.stage1 import Stage1Engine

    vp, lp = W.siglip_vision_params(cfg.vision), W.gemma3_params(cfg.text)
    pp = W.projector_params(cfg.vision.hidden_size, cfg.text.hidden_size)
    px, ids, labels = (torch.from_numpy(t).to(gpu) for t in W.synthetic_batch(cfg, seed=5))

    def one_step(switch):
        monkeypatch.setenv("PTK_B_KTILED", switch)
        proj = MLPProjector(cfg.vision.hidden_size, cfg.text.hidden_size)
        proj.load_state_dict({k: torch.from_numpy(v) for k, v in pp.items()})
        proj.to(gpu)
        vis = SiglipVisionTower(cfg.vision, vp, gpu)
        llm = Gemma3CausalLM(cfg.text, lp, gpu, max_pos=Gemma3CausalLM.seq_pad(cfg.seq_len))
        packed = [lay["kt"][k] is not None for lay in vis.layers for k in lay["kt"]]
        packed += [lay[k] is not None for lay in llm.layers for k in lay if k.endswith("_kt")]
        assert all(packed) if switch == "1" else not any(packed)
        eng = Stage1Engine(vis, llm, proj)
        loss = eng.step(px, ids, labels)
        torch.cuda.synchronize()
        return loss.clone(), eng.grad_norm.clone(), eng.proj.flat_grad.clone()

    on, _ = _forced(L, mode, lambda: one_step("1"))
    off, _ = _forced(L, mode, lambda: one_step("0"))
    assert torch.isfinite(on[0]).all() and float(on[1]) > 0
    return on, off


@pytest.mark.parametrize("mode", [0, 32])
def test_tiny_stage1_step_packing_on_off(gpu, monkeypatch, mode):
    """One tiny Stage-1 step with packing on and off: loss, grad norm and projector grads bit-identical; under the
    default dispatch and with every GEMM forced onto the persistent 8-wave kernel where it is supported (the tiny
    shapes' default dispatch takes no persistent kernel)."""
    from projectiontrainer_amd.config import PRESETS
    on, off = _stage1_step_on_off(gpu, monkeypatch, PRESETS["tiny"], mode)
    for a, b in zip(on, off):
        assert torch.equal(a, b)


@pytest.mark.parametrize("mode", [0, 32])
def test_k_sliced_frozen_gemms_read_row_major(gpu, monkeypatch, mode):
    """K slices must not take the tiled pointer.  A Gemma3 of hidden 512 / intermediate 1 024 on 192 token rows: few
    128x128 tiles, so gemm_split cuts the frozen-weight projections that carry a tiled copy along K (asserted through
    ptk_gemm_split_plan for the down projection, K 1 024, and d(gate|up) dX, K 2 048); the slices are launches over a
    part of each row of B, which only row-major B can serve.  One Stage-1 step with packing on and off is
    bit-identical, under the default dispatch and with the slice launches forced onto the 8-wave kernel."""
    from projectiontrainer_amd import _lib as L
    from projectiontrainer_amd.config import SIGLIP_TINY, Gemma3TextConfig, Stage1Config
    from projectiontrainer_amd.gemma3 import Gemma3CausalLM
    text = Gemma3TextConfig(vocab_size=512, hidden_size=512, intermediate_size=1024, num_hidden_layers=2,
                            num_attention_heads=2, num_key_value_heads=1, head_dim=64, sliding_window=8,
                            sliding_window_pattern=2, query_pre_attn_scalar=64)
    cfg = Stage1Config(vision=SIGLIP_TINY, text=text, batch_size=3, text_len=16)
    M = cfg.batch_size * Gemma3CausalLM.seq_pad(cfg.seq_len)
    ncu = torch.cuda.get_device_properties(gpu).multi_processor_count
    for N, K in ((text.hidden_size, text.intermediate_size), (text.hidden_size, 2 * text.intermediate_size)):
        d = L.GemmDesc()
        d.M, d.N, d.K, d.lda, d.ldb, d.ldc = M, N, K, K, K, N
        d.alpha, d.act, d.out, d.batch = 1.0, L.ACT_NONE, L.OUT_BF16, 1
        sl, kc = L.C.c_int(), L.C.c_int()
        part = L.lib().ptk_gemm_tail_scratch_bytes() // 4 + 64   # the model workspace's split-K scratch is at least this
        assert L.lib().ptk_gemm_split_plan(d, ncu, part, L.C.byref(sl), L.C.byref(kc), None, None) == 0
        assert sl.value > 1 and 0 < kc.value < K, (M, N, K, sl.value, kc.value)
    on, off = _stage1_step_on_off(gpu, monkeypatch, cfg, mode)
    for a, b in zip(on, off):
        assert torch.equal(a, b)
