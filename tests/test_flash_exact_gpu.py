"""Flash attention kernels (csrc/flash.hip) against a float64 reference on inputs from which a fault can be read
exactly; references, input builders, checkers and the bars are in tests/flash_util.py, and
tests/test_flash_checks_cpu.py proves on the CPU that they see the faults they are meant for.

  F1  forward mask readout, hd 256 (attn_fwd256w, and the generic kernel past 4096 keys): one-hot V
  F2  forward readout, hd 64 (attn_fwd64), fused qkv layout and causal GQA
  F3  decode shapes: rows = G, K / V views into a cache whose other rows are bait
  F4  dynamic range: Q = a I with score rows that force the deferred-max rescale, forward and backward
  F5  backward readout: Q = a I / K = a e_k with one-hot dO (dK = dS^T, dV = P^T, dQ = dS)
  F6  persistence: more work items than CUs, bit-equal to launches of one sample each
  F7  per-row numerics at the model's shapes

FLASH_EXACT_REPORT=<file>: every test appends its worst ratios (profiles/flash_exact_gpu.txt is such a run)."""
import os
from types import SimpleNamespace

import pytest
import torch

from tests import flash_util as U

pytestmark = pytest.mark.gpu


def _kn():
    from projectiontrainer_amd import kernels as Kn
    return Kn


def _nan(*shape, dev, dtype=torch.bfloat16):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def _common(c):
    return dict(rows=c.rows, nkeys=c.nkeys, head_dim=c.D, batch=c.Z, batch_inner=c.Hkv, zdiv=c.Hkv, qdiv=c.G,
                causal=c.causal, window=c.window, key_valid=c.key_valid, scale=c.scale)


def forward(c, layout="plain"):
    """The forward kernel on a device-resident case -> (O [Z, rows, D] bf16, LSE [Z, rows] fp32); outputs prefilled
    with NaN so an unwritten element shows.  layout "token": O token-major through the row map as in the model
    ([B * S, Hq * D], omap = (G, 0, Hq, 0)); "fused": Q | K | V read in place from one [B * N, 3 * H * D] buffer;
    "cache": K / V views at c.offset into c.Kcache / c.Vcache."""
    Kn, dev = _kn(), c.Q.device
    Z, rows, nk, D, Hkv, G = c.Z, c.rows, c.nkeys, c.D, c.Hkv, c.G
    lse = _nan(Z, rows, dev=dev, dtype=torch.float32)
    cm = _common(c)
    if layout == "fused":
        assert G == 1 and rows == nk
        B, W = c.B, Hkv * D
        qkv = torch.stack([c.Q, c.K, c.V]).view(3, B, Hkv, rows, D).permute(1, 3, 0, 2, 4).reshape(B * rows, 3 * W).contiguous()
        O = _nan(B * rows, W, dev=dev)
        Kn.flash_attn(qkv, qkv[:, W:], qkv[:, 2 * W:], O, lse=lse, ldq=3 * W, ldk=3 * W, ldo=W,
                      strides=(rows * 3 * W, D, rows * 3 * W, D, rows * W, D), **cm)
        return O.view(B, rows, Hkv, D).permute(0, 2, 1, 3).reshape(Z, rows, D), lse
    Q = c.Q.contiguous()
    sq = (Hkv * rows * D, rows * D)
    if layout == "cache":
        Smax = c.Kcache.shape[1]
        K, V, sk = c.Kcache[:, c.offset:], c.Vcache[:, c.offset:], (Hkv * Smax * D, Smax * D)
    else:
        K, V, sk = c.K.contiguous(), c.V.contiguous(), (Hkv * nk * D, nk * D)
    if layout == "token":
        S, Hq = rows // G, Hkv * G
        assert S * G == rows
        O = _nan(c.B * S, Hq * D, dev=dev)
        Kn.flash_attn(Q, K, V, O, lse=lse, ldq=D, ldk=D, ldo=D, strides=(*sq, *sk, S * Hq * D, G * D), omap=(G, 0, Hq, 0), **cm)
        return O.view(c.B, S, Hkv, G, D).permute(0, 2, 1, 3, 4).reshape(Z, rows, D), lse
    O = _nan(Z, rows, D, dev=dev)
    Kn.flash_attn(Q, K, V, O, lse=lse, ldq=D, ldk=D, ldo=D, strides=(*sq, *sk, *sq), **cm)
    return O, lse


def backward(c, O, lse, split=True):
    dQ, dK, dV = _kn().flash_attn_bwd(c.Q.contiguous(), c.K.contiguous(), c.V.contiguous(), O.contiguous(), c.dO.contiguous(), lse,
                                      sO=(c.Hkv * c.rows * c.D, c.rows * c.D), split=split, **_common(c))
    return dQ, dK, dV


def run(fam, c, dev, layout="plain", bwd=False, split=True):
    """Kernels and float64 reference of one case on the device; every check of the family; the ratios reported."""
    c = U.to(c, dev)
    got = SimpleNamespace()
    got.O, got.LSE = forward(c, layout)
    if bwd:
        got.dQ, got.dK, got.dV = backward(c, got.O, got.LSE, split)
    torch.cuda.synchronize()
    m = U.case_mask(c, dev)
    ref = U.ref_of(c)
    worst = U.check_family(fam, c, ref, got, m)
    _report(fam, c.name + ("" if split else " nosplit"), worst)
    return c, ref, got, m


def _report(fam, name, worst):
    line = f"{fam} {name}: " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items())
    print(line)
    path = os.environ.get("FLASH_EXACT_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


# ------------------------------------------------------------------------------------------------ F1
@pytest.mark.parametrize("window", U.F1_WINDOWS)
def test_f1_fwd_mask_readout(gpu, window):
    """Hkv 1, G 4, S 320, B 2; sample 0 left-padded by 70 keys (two whole tiles + 6: positions 0..69 are fully masked
    rows), sample 1 with a hole and a masked tail.  Up to window 255 a row's visible keys span fewer than 256 classes,
    so O is the P row itself and a key beyond either window edge lands on an exact zero; at 256 and at 0 the classes
    fold and the sums are compared (empty classes still exact zeros)."""
    run("F1", U.f1_case(4, 320, window), gpu, layout="token")


@pytest.mark.parametrize("G,S", U.F1_SHAPES[1:])
@pytest.mark.parametrize("window", (0, 33))
def test_f1_fwd_mask_readout_partial_blocks(gpu, G, S, window):
    """Query rows that are no multiple of the 128-row block: G 3 / S 300 (900 rows), G 1 / S 36 (idle waves)."""
    run("F1", U.f1_case(G, S, window), gpu, layout="token")


def test_f1_fwd_generic_kernel_readout(gpu):
    """4128 keys: past the mask table, the generic forward kernel."""
    run("F1", U.generic_fwd_case(), gpu)


# ------------------------------------------------------------------------------------------------ F2
@pytest.mark.parametrize("N", U.F2_N)
def test_f2_fwd64_fused_layout_readout(gpu, N):
    run("F2", U.f2_case(N=N), gpu, layout="fused")


@pytest.mark.parametrize("window", U.F2_WINDOWS)
def test_f2_fwd64_causal_readout(gpu, window):
    run("F2", U.f2_case(window=window), gpu)


# ------------------------------------------------------------------------------------------------ F3
@pytest.mark.parametrize("G", U.F3_G)
@pytest.mark.parametrize("nkeys,with_kv", [(n, False) for n in U.F3_NKEYS] + [(n, True) for n in U.F3_NKEYS_KV])
def test_f3_decode_shapes(gpu, G, nkeys, with_kv):
    """rows = G, non-causal, K / V at an offset into a cache; every cache row outside [offset, offset + nkeys) is bait
    (a dominating score, V classes no real key uses): those classes must read exactly 0."""
    c, ref, got, m = run("F3", U.decode_case(G, nkeys, with_kv), gpu, layout="cache")
    assert bool((got.O[..., c.D - 16:] == 0).all())


# ------------------------------------------------------------------------------------------------ F4
@pytest.mark.parametrize("D,causal,nkeys", U.F4_CASES)
def test_f4_dynamic_range(gpu, D, causal, nkeys):
    """Score rows that move the running max at every tile, just under / over FA_DEFER, never, and by 40 log2 units on
    the last key (event counts asserted in tests/test_flash_checks_cpu.py): O and LSE, then the backward."""
    run("F4", U.dynrange_case(D, causal, nkeys), gpu, bwd=True)


# ------------------------------------------------------------------------------------------------ F5
@pytest.mark.parametrize("split", (True, False))
@pytest.mark.parametrize("window", U.F5_WINDOWS)
@pytest.mark.parametrize("D,S,G", U.F5_SHAPES)
def test_f5_bwd_readout_dk_dv(gpu, D, S, G, window, split):
    """Q = a I, dO one-hot by row: dK[k][q] = dS[q, k], dV[k][q] = P[q, k]; masked pairs exact zeros.  G 3: the generic
    dK / dV kernel."""
    run("F5", U.bwd_readout_case(D, S, G, window), gpu, bwd=True, split=split)


@pytest.mark.parametrize("split", (True, False))
@pytest.mark.parametrize("window", U.F5_WINDOWS)
@pytest.mark.parametrize("D,S,G", U.F5_DUAL)
def test_f5_bwd_readout_dq(gpu, D, S, G, window, split):
    """K = a e_k: dQ[q][k] = dS[q, k]."""
    run("F5", U.bwd_readout_case(D, S, G, window, kind="kI"), gpu, bwd=True, split=split)


# ------------------------------------------------------------------------------------------------ F6
@pytest.mark.parametrize("window", U.F6_WINDOWS)
def test_f6_persistent_items(gpu, window):
    """hd 256, S 64, G 4 (two row blocks per z), Hkv 2, B such that the forward and dQ kernels have at least 1.25
    work items per CU: every workgroup walks more than one item, with the next item's key masks, Q and first tiles
    issued before the current epilogue.  Per z: the row checks, and O, LSE and dQ bit-equal to the same sample
    launched alone (4 items).  dK / dV are exempt: their slab plan depends on nz."""
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    B = -(-5 * cus // 16)                     # 2 row blocks x 2 B z >= 1.25 cus
    assert 2 * (2 * B) >= 1.25 * cus
    c, ref, got, m = run("F6", U.persist_case(B, window), gpu, bwd=True)
    for b in range(B):
        z = slice(2 * b, 2 * b + 2)
        one = SimpleNamespace(**{**vars(c), "Z": 2, "B": 1, "Q": c.Q[z], "K": c.K[z], "V": c.V[z], "dO": c.dO[z],
                                 "key_valid": c.key_valid[b:b + 1].contiguous()})
        O1, lse1 = forward(one)
        dQ1, _, _ = backward(one, O1, lse1)
        assert torch.equal(O1, got.O[z]), b
        assert torch.equal(lse1, got.LSE[z]), b
        assert torch.equal(dQ1, got.dQ[z]), b


# ------------------------------------------------------------------------------------------------ F7
@pytest.mark.parametrize("S,window,B", U.F7_CASES)
def test_f7_rows_at_model_shapes(gpu, S, window, B):
    """cfg2's sliding and global layers (S 704) and the default caption length (S 1088): every output row of O, dQ, dK
    and dV within the per-row bar, beside test_flash_bwd_vs_autograd's whole-tensor norm."""
    run("F7", U.random_case(256, 1, 4, S, B, window), gpu, layout="token", bwd=True)
