"""The two-kernel input-embedding gradient (train.hip embed_rank_kernel + embed_grad_kernel) through its unit-test
surface ptk_embed_grad, against a plain CPU reference: per id, the rows' bf16(bf16(dx_row) * escale) added in
fp32 one row at a time in ascending position order, then dE[id] = bf16(dE[id] + bf16(acc)).  The kernel adds in
the same order and every product is rounded before its add (nothing to contract), so the whole of dE -- rows of
unused ids included -- must be bit-equal.

The shapes reach what the tiny and cfg4-width presets do not: n no multiple of 64 and more than one 1024-key
tile in the rank kernel; runs of one id of exactly 256 and of more (the second count pass), of exactly 2048 and
of more (a second staging chunk), run lengths that are no multiple of the 8-row unroll; H > 1280 (a second
column pass, cfg5's 2560) and H that is no multiple of 256 (clamped loads)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
NV = 3          # vision rows in front of the text rows
PAD_ID = 0


def ids_tiny():
    """2 x 20, mostly distinct ids of a 512 vocabulary (two repeats, one across the samples)."""
    gen = torch.Generator().manual_seed(1)
    ids = torch.randperm(512, generator=gen)[:40].clone()
    ids[7], ids[33] = ids[5], ids[5]
    ids[21] = ids[20]
    return ids.view(2, 20), 512


def ids_cfg4():
    """4 x 275 = 1100 (> 1024 keys: two rank tiles; 1100 % 64 = 12): vocabulary 50, the pad id on 300 positions
    (second count pass, 300 % 8 = 4), id 1 on exactly 256, id 49 present, ids 2..48 on the other 543."""
    gen = torch.Generator().manual_seed(2)
    ids = torch.cat([torch.full((300,), PAD_ID), torch.full((256,), 1), torch.tensor([49]),
                     torch.randint(2, 49, (543,), generator=gen)])
    ids = ids[torch.randperm(1100, generator=gen)]
    assert int((ids == PAD_ID).sum()) == 300 and int((ids == 1).sum()) == 256 and int((ids == 49).sum()) == 1
    return ids.view(4, 275), 50


def ids_cfg5():
    """4 x 625 = 2500 (three rank tiles; 2500 % 64 = 4): the pad id on 2100 positions (one staging chunk of 2048
    and 52 more, 52 % 8 = 4), the rest distinct ids of the 262 144 vocabulary, the last one among them."""
    gen = torch.Generator().manual_seed(3)
    rest = torch.randperm(262_143, generator=gen)[:399] + 1          # 1 .. 262 143, distinct
    rest = rest[rest != 262_143][:398]
    ids = torch.cat([torch.full((2100,), PAD_ID), rest, torch.full((400 - len(rest),), 262_143)])
    ids = ids[torch.randperm(2500, generator=gen)]
    assert int((ids == PAD_ID).sum()) == 2100 and int((ids == 262_143).sum()) >= 1 and len(ids) == 2500
    return ids.view(4, 625), 262_144


def ids_chunk():
    """4 x 640 = 2560 (a multiple of 64): one id on exactly 2048 positions (one full staging chunk, eight full
    count passes and an empty ninth), the other 512 distinct."""
    gen = torch.Generator().manual_seed(4)
    rest = torch.randperm(4095, generator=gen)[:513]
    rest = rest[rest != 777][:512]
    ids = torch.cat([torch.full((2048,), 777), rest])
    ids = ids[torch.randperm(2560, generator=gen)]
    assert int((ids == 777).sum()) == 2048
    return ids.view(4, 640), 4096


CASES = {"tiny_H128": (ids_tiny, 128), "cfg4_H1152": (ids_cfg4, 1152), "cfg5_H2560": (ids_cfg5, 2560),
         "chunk_H1288": (ids_chunk, 1288)}


def embed_grad(ids, B, T, Sp, H, escale, dx, dE, ws, ws_bytes=None):
    from projectiontrainer_amd import _lib as L
    return L.lib().ptk_embed_grad(ids.data_ptr(), B, T, NV, Sp, H, escale, dx.data_ptr(), dE.data_ptr(),
                                  ws.data_ptr(), ws.numel() if ws_bytes is None else ws_bytes,
                                  L.stream_ptr(dE.device))


def reference_rows(ids, dx, dE_rows, escale, Sp):
    """{id: new dE row} on the CPU: one row at a time in position order, vectorised over H only."""
    B, T = ids.shape
    esc = torch.tensor(escale, dtype=torch.float32)
    flat = ids.reshape(-1).tolist()
    acc = {}
    for j, tok in enumerate(flat):                       # ascending position
        b, t = divmod(j, T)
        r = (dx[b * Sp + NV + t].bfloat16().float() * esc).bfloat16().float()
        acc[tok] = acc[tok] + r if tok in acc else torch.zeros_like(r) + r
    return {tok: (dE_rows[tok].float() + a.bfloat16().float()).bfloat16() for tok, a in acc.items()}


@pytest.mark.parametrize("case", list(CASES))
def test_embed_grad_bit_equal_to_reference(gpu, case):
    from projectiontrainer_amd import _lib as L
    make_ids, H = CASES[case]
    ids, vocab = make_ids()
    B, T = ids.shape
    Sp = T + 8
    escale = float(torch.tensor(float(H) ** 0.5).bfloat16())     # Gemma's embedding scale, a bf16 value
    gen = torch.Generator().manual_seed(11 + H)
    dx = torch.full((B * Sp, H), float("nan"))                    # a wrong row index shows
    text = (torch.arange(B).view(B, 1) * Sp + NV + torch.arange(T).view(1, T)).reshape(-1)
    dx[text] = torch.randn(B * T, H, generator=gen) * 0.01
    # dE pre-filled with non-zero bf16 on the device (the 262 144 x 2560 table never visits the host); only the
    # rows of ids that occur come back for the reference
    dE = torch.empty(vocab, H, dtype=torch.bfloat16, device=gpu).uniform_(0.001, 0.02)
    dE[::2].neg_()
    assert bool((dE != 0).all())
    used = torch.unique(ids)
    rows0 = dict(zip(used.tolist(), dE[used.to(gpu)].cpu()))
    want = dE.clone()
    new = reference_rows(ids, dx, rows0, escale, Sp)
    want[used.to(gpu)] = torch.stack([new[t] for t in used.tolist()]).to(gpu)
    nbytes = L.lib().ptk_embed_grad_workspace_bytes(B, T)
    assert nbytes >= 8 * B * T
    ws = torch.empty(nbytes, dtype=torch.uint8, device=gpu)
    rc = embed_grad(ids.to(gpu), B, T, Sp, H, escale, dx.to(gpu), dE, ws)
    assert rc == 0, L.lib().ptk_last_error()
    torch.cuda.synchronize()
    got, ref = dE.view(torch.int16), want.view(torch.int16)
    bad_rows = (got != ref).any(dim=1).nonzero().flatten().tolist()
    assert not bad_rows, f"{len(bad_rows)} rows of dE differ, first ids {bad_rows[:8]} (used: " \
                         f"{[r in set(used.tolist()) for r in bad_rows[:8]]})"
    assert not bool(torch.isnan(dE[used.to(gpu)].float()).any())


def test_embed_grad_no_tokens_is_a_no_op(gpu):
    dE = torch.empty(16, 128, dtype=torch.bfloat16, device=gpu).uniform_(0.5, 1.0)
    keep = dE.clone()
    ids = torch.zeros(4, dtype=torch.int64, device=gpu)
    dx = torch.full((32, 128), float("nan"), device=gpu)
    ws = torch.empty(64, dtype=torch.uint8, device=gpu)
    for B, T in ((0, 4), (4, 0)):
        assert embed_grad(ids, B, T, T + 8, 128, 1.0, dx, dE, ws) == 0
    torch.cuda.synchronize()
    assert torch.equal(dE.view(torch.int16), keep.view(torch.int16))
