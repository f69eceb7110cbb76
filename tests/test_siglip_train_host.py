"""The trained SigLIP tower's C ABI and the engine's flag logic, on a machine without a GPU: exported symbols,
the training workspace's size, the host-side refusals (which come before any launch, so they answer without a
device) and Stage2Engine's "nothing trainable" check."""
import ctypes
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptk.h")

NEW_SYMBOLS = ["ptk_siglip_train_workspace_bytes", "ptk_siglip_train_fwd", "ptk_siglip_bwd",
               "ptk_layernorm_bwd_partial_floats", "ptk_layernorm_bwd_bf16", "ptk_gelu_tanh_bwd_bf16",
               "ptk_colsum_bf16_acc", "ptk_pos_grad_bf16", "ptk_projector_input_grad_workspace_bytes",
               "ptk_projector_input_grad"]


def lib():
    from projectiontrainer_amd import _lib as L
    return L, L.lib()


def siglip_c(image=384, hidden=1024, heads=16, inter=4096, layers=24):
    L, _ = lib()
    return L.SiglipConfigC(image, 16, 3, hidden, heads, inter, layers, 1e-6)


def test_new_symbols_are_exported_and_the_abi_version_stays():
    L, l = lib()
    header = open(HEADER).read()
    for n in NEW_SYMBOLS:
        assert hasattr(l, n), n
        assert n in L.SIGNATURES, n
        assert n + "(" in header, n
    assert l.ptk_abi_version() == L.ABI_VERSION == 8      # additions only


def test_grads_struct_layouts_match_c_compiler():
    L, _ = lib()
    structs = {"ptk_siglip_layer_grads": L.SiglipLayerGradsC, "ptk_siglip_grads": L.SiglipGradsC}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for fname, _t in cls._fields_:
            lines.append(f'printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write("\n".join(lines))
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-o", exe, c])
        got = {tuple(ln.split()[:2]): int(ln.split()[2]) for ln in subprocess.check_output([exe]).decode().split("\n")
               if ln}
    for cname, cls in structs.items():
        assert ctypes.sizeof(cls) == got[(cname, "sizeof")], cname
        for fname, _t in cls._fields_:
            assert getattr(cls, fname).offset == got[(cname, fname)], (cname, fname)


def test_train_workspace_size_at_l16_384():
    """>= the frozen forward's at batch 1 and 32, affine in the batch, and at batch 32 within the derived budget of
    the saved activations -- 2 M (8 D + 2 I) bytes per layer, M = 18 432, 24 layers: 14.5 GB -- with a 25 % margin
    for the backward's scratch."""
    _, l = lib()
    c = siglip_c()
    D, I, M = 1024, 4096, 32 * 576
    train = {b: l.ptk_siglip_train_workspace_bytes(c, b) for b in (1, 2, 3, 16, 32)}
    for b in (1, 32):
        assert train[b] >= l.ptk_siglip_workspace_bytes(c, b) > 0
    step = train[2] - train[1]
    assert step > 0
    # (every buffer's start is rounded up to 256 bytes: a few KiB of slack over ~200 buffers)
    assert abs((train[3] - train[2]) - step) <= 1 << 16
    assert abs((train[32] - train[16]) - 16 * step) <= 1 << 20
    budget = 24 * 2 * M * (8 * D + 2 * I)
    print(f"train workspace at L/16-384 batch 32: {train[32] / 1e9:.2f} GB (budget {budget / 1e9:.2f} GB)")
    assert train[32] <= 1.25 * budget
    assert train[32] >= 24 * 2 * M * (6 * D + 2 * I)      # what the backward reads is really kept


@pytest.mark.parametrize("entry", ["ptk_siglip_train_fwd", "ptk_siglip_bwd"])
def test_refusals_come_before_any_launch(entry):
    """196 patches, head_dim 32 and a short workspace: -1 with a message that names the limit.  Every pointer is
    NULL and there may be no device at all, so nothing can have been launched."""
    L, l = lib()
    fn = getattr(l, entry)

    def call(c, ws_bytes=0):
        if entry == "ptk_siglip_train_fwd":
            return fn(c, None, 1, None, None, None, ws_bytes, None)
        return fn(c, None, 1, None, None, None, ws_bytes, None)

    assert call(siglip_c(image=224, hidden=768, heads=12, inter=3072, layers=12)) == -1
    msg = l.ptk_last_error().decode()
    assert "num_patches 196" in msg and "multiple of 64" in msg, msg
    assert call(siglip_c(image=128, hidden=128, heads=4, inter=256, layers=2)) == -1
    msg = l.ptk_last_error().decode()
    assert "head_dim 32" in msg and "64" in msg, msg
    ok = siglip_c(image=128, hidden=128, heads=2, inter=256, layers=2)
    need = l.ptk_siglip_train_workspace_bytes(ok, 1)
    assert call(ok, need - 1) == -1
    assert "workspace too small" in l.ptk_last_error().decode()


def test_kernel_entries_validate_before_any_launch():
    L, l = lib()
    assert l.ptk_layernorm_bwd_bf16(None, None, None, None, None, 4, 100, 1e-6, None, None, None, 0, None) == -1
    assert "multiple of 8" in l.ptk_last_error().decode()
    assert l.ptk_layernorm_bwd_bf16(None, None, None, None, None, 4, 4096, 1e-6, None, None, None, 0, None) == -1
    assert l.ptk_gelu_tanh_bwd_bf16(None, None, None, 4, 12, None) == -1
    assert l.ptk_layernorm_bwd_partial_floats(18432, 1152) >= 2 * (18432 // 32) * 1152


def test_engine_with_nothing_trainable_is_a_value_error():
    """train_llm, train_projector and train_vision all False: the constructor's first check, before any device
    work (the towers are dummies); train_vision is a keyword the engine knows."""
    from projectiontrainer_amd.stage2 import Stage2Engine
    with pytest.raises(ValueError, match="No trainable parameters found"):
        Stage2Engine(object(), object(), object(), train_llm=False, train_projector=False, train_vision=False)
    with pytest.raises(ValueError, match="No trainable parameters found"):
        Stage2Engine(object(), object(), object(), train_llm=False, train_projector=False)
