"""Records what the token-selection entry points (ptk_sample_next_token, ptk_beam_candidates,
ptk_beam_candidates_penalized) return for a fixed list of cases, bit for bit, and the Gemma3 workspace sizes:

    tools/build_prev.sh <parent>
    PTK_LIB=build/libptk_prev.so python tools/selection_table.py        # -> tests/golden/selection_parent.npz

tests/test_selection_parent_gpu.py reruns every case on the in-tree library and compares every recorded array;
tests/test_workspace_parent.py compares the workspace sizes (no GPU).  The inputs of a case are generated on the CPU
from a torch generator seeded per case, so the fixture holds outputs only.  Recording runs every case twice and
refuses to write if the two runs differ.  Importing this module touches neither the environment nor the library.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "selection_parent.npz")

EOS, PAD = 7, 3          # the sampling cases' eos / pad ids
SENTINEL = -7            # outputs start as this (a call that fails validation writes nothing)
SAMPLE_ROWS = 5          # row 2 draws EOS (a spike at token EOS), row 3 arrives finished
PEN_VARIANTS = [(1.8, 1), (1.8, 70), (0.6, 1), (0.6, 70)]


def _case(cid, kind, V, paths, **kw):
    c = dict(id=cid, kind=kind, V=V, ld_extra=0, logits="normal", do_sample=0, top_k=0, top_p=1.0, temperature=1.0,
             step=0, penalty=1.0, n_hist=0, K=3, n_cand=6, min_keep=1, batch=2, penalized_entry=False,
             paths=set(paths))
    c.update(kw)
    if c["ld_extra"]:
        c["paths"].add("unaligned_rows")
    c["paths"].add(f"V{V}")
    return c


def _with_penalties(base):
    """base and its four penalised repeats (p in {1.8, 0.6} x n_hist in {1, 70})."""
    out = [base]
    for p, n in PEN_VARIANTS:
        c = dict(base, id=f"{base['id']}.p{p}.h{n}", penalty=p, n_hist=n, penalized_entry=True)
        c["paths"] = set(base["paths"]) | {"penalty", f"pen_p{p}", f"pen_h{n}"}
        out.append(c)
    return out


def cases():
    cs = []
    shapes = [(256, 0), (1000, 3), (4104, 0), (262144, 0)]   # (V, ld - V)
    # ---- ptk_sample_next_token
    for i, (V, ex) in enumerate(shapes):
        cs += _with_penalties(_case(f"sample.greedy.V{V}", "sample", V, ["sample.greedy"], ld_extra=ex, step=5 * (i % 2)))
        cs += _with_penalties(_case(f"sample.k50p09.V{V}", "sample", V, ["sample.k50_p0.9", f"sample.step{5 * ((i + 1) % 2)}"],
                                    ld_extra=ex, do_sample=1, top_k=50, top_p=0.9, step=5 * ((i + 1) % 2),
                                    temperature=0.7 if V == 4104 else 1.0))
    for V, ex in shapes[1:]:
        cs.append(_case(f"sample.k50p1.V{V}", "sample", V, ["sample.k50_p1_sorted_draw"], ld_extra=ex, do_sample=1,
                        top_k=50, step=5))
    cs.append(_case("sample.k0p1.V256", "sample", 256, ["sample.k0_p1_small_vocab_sorted_draw"], do_sample=1))
    for V in (4104, 262144):
        cs.append(_case(f"sample.k0p1.V{V}", "sample", V, ["sample.chunked_draw_no_threshold"], do_sample=1, step=5))
        cs.append(_case(f"sample.k600p1.V{V}", "sample", V, ["sample.chunked_draw_threshold"], do_sample=1, top_k=600))
    cs.append(_case("sample.t07.k50p1.V4104", "sample", 4104, ["sample.temperature"], do_sample=1, top_k=50,
                    temperature=0.7))
    cs.append(_case("sample.ties.V4104", "sample", 4104, ["sample.ties_at_top_k"], logits="quantised", do_sample=1,
                    top_k=50, top_p=0.9))
    cs.append(_case("sample.overflow.V4104", "sample", 4104, ["sample.overflow_argmax_fallback"], logits="const_row0",
                    do_sample=1, top_k=50, top_p=0.9))
    cs.append(_case("sample.overflow.pen.V4104", "sample", 4104, ["sample.overflow_penalised_error", "penalty"],
                    logits="const_row0", do_sample=1, top_k=50, top_p=0.9, penalty=1.8, n_hist=1))
    cs.append(_case("sample.forward.p1.8.h0.V1000", "sample", 1000, ["sample.forward_empty_history"], do_sample=1,
                    top_k=50, top_p=0.9, penalty=1.8, n_hist=0))
    cs.append(_case("sample.forward.p1.h70.V1000", "sample", 1000, ["sample.forward_penalty_one"], do_sample=1,
                    top_k=50, top_p=0.9, penalty=1.0, n_hist=70))
    # ---- ptk_beam_candidates(_penalized)
    for i, (V, ex) in enumerate(shapes):
        cs += _with_penalties(_case(f"beam.greedy.K3.V{V}", "beam", V, ["beam.greedy", "beam.K3"], ld_extra=ex, step=i))
        cs += _with_penalties(_case(f"beam.k50p09m2.K3.V{V}", "beam", V, ["beam.k50_p0.9_min_keep2", "beam.K3"],
                                    ld_extra=ex, do_sample=1, top_k=50, top_p=0.9, min_keep=2, step=i + 1,
                                    temperature=0.7 if V == 4104 else 1.0))
    cs += _with_penalties(_case("beam.greedy.K1.V1000", "beam", 1000, ["beam.greedy", "beam.K1"], K=1))
    cs += _with_penalties(_case("beam.k50p09m2.K1.V4104", "beam", 4104, ["beam.k50_p0.9_min_keep2", "beam.K1"], K=1,
                                do_sample=1, top_k=50, top_p=0.9, min_keep=2, step=2))
    for V, ex in shapes[1:]:
        cs.append(_case(f"beam.k50p1.K3.V{V}", "beam", V, ["beam.k50_p1"], ld_extra=ex, do_sample=1, top_k=50, step=3))
    cs.append(_case("beam.ties.V4104", "beam", 4104, ["beam.ties_at_top_k"], logits="quantised", do_sample=1, top_k=50,
                    top_p=0.9, min_keep=2))
    cs.append(_case("beam.overflow.V4104", "beam", 4104, ["beam.overflow_no_candidates"], logits="const_row0",
                    do_sample=1, top_k=50, top_p=0.9, min_keep=2))
    cs.append(_case("beam.overflow.pen.V4104", "beam", 4104, ["beam.overflow_penalised_error", "penalty"],
                    logits="const_row0", do_sample=1, top_k=50, top_p=0.9, min_keep=2, penalty=1.8, n_hist=1,
                    penalized_entry=True))
    cs.append(_case("beam.forward.p1.8.h0.V1000", "beam", 1000, ["beam.forward_empty_history"], do_sample=1, top_k=50,
                    top_p=0.9, min_keep=2, penalty=1.8, n_hist=0, penalized_entry=True))
    cs.append(_case("beam.forward.p1.h70.V1000", "beam", 1000, ["beam.forward_penalty_one"], do_sample=1, top_k=50,
                    top_p=0.9, min_keep=2, penalty=1.0, n_hist=70, penalized_entry=True))
    ids = [c["id"] for c in cs]
    assert len(set(ids)) == len(ids)
    return cs


# every path the case list must reach, by name (the test asserts the list still covers them)
REQUIRED_PATHS = {
    "V256", "V1000", "V4104", "V262144", "unaligned_rows",
    "sample.greedy", "sample.k50_p0.9", "sample.k50_p1_sorted_draw", "sample.k0_p1_small_vocab_sorted_draw",
    "sample.chunked_draw_no_threshold", "sample.chunked_draw_threshold", "sample.temperature", "sample.step0",
    "sample.step5", "sample.ties_at_top_k", "sample.overflow_argmax_fallback", "sample.overflow_penalised_error",
    "sample.forward_empty_history", "sample.forward_penalty_one",
    "beam.greedy", "beam.k50_p0.9_min_keep2", "beam.k50_p1", "beam.K3", "beam.K1", "beam.ties_at_top_k",
    "beam.overflow_no_candidates", "beam.overflow_penalised_error", "beam.forward_empty_history",
    "beam.forward_penalty_one",
    "penalty", "pen_p1.8", "pen_p0.6", "pen_h1", "pen_h70",
}


def make_inputs(c):
    """The case's CPU inputs: bf16 logits [rows, V] (a view of [rows, V + ld_extra]), and by kind the finished flags,
    beam scores and histories.  Histories hold a repeat, the row's arg-max (so the penalty moves the top of the
    row) and, in row 0, one id outside [0, V)."""
    import torch
    g = torch.Generator().manual_seed(1000 + sum(ord(ch) * (i + 1) for i, ch in enumerate(c["id"])) % 100000)
    V = c["V"]
    rows = SAMPLE_ROWS if c["kind"] == "sample" else c["batch"] * c["K"]
    x = torch.randn(rows, V, generator=g) * 3.0
    if c["logits"] == "quantised":   # about 40 distinct bf16 values: the kept set exceeds top_k, under the capacity
        x = torch.round(x * 3.0) / 3.0
        x = x.clamp(-6.5, 6.5)
    if c["logits"] == "const_row0":  # more than 1 024 entries tie at the top-k boundary
        x[0] = 0.5
    if c["kind"] == "sample":
        x[2] -= 20.0
        x[2, EOS] = 40.0             # row 2 draws EOS whatever the warpers and the penalty do
    buf = torch.zeros(rows, V + c["ld_extra"], dtype=torch.bfloat16)
    buf[:, :V] = x.to(torch.bfloat16)
    inp = {"logits": buf, "rows": rows}
    if c["kind"] == "sample":
        fin = torch.zeros(rows, dtype=torch.int32)
        fin[3] = 1
        inp["finished"] = fin
    else:
        inp["beam_scores"] = -torch.rand(rows, generator=g) * 4.0
    n = c["n_hist"]
    if n > 0:
        h = torch.randint(0, V, (rows, n), generator=g, dtype=torch.int64)
        top = buf[:, :V].float().argmax(dim=1)
        h[1:, 0] = top[1:]
        if n >= 3:
            h[:, 2] = h[:, 1]        # a repeat
            h[:, n // 2] = top       # (row 0 too)
        h[0, n - 1] = V + 5          # outside the vocabulary
        inp["history"] = h
    return inp


def run_case(c, dev):
    """One call of the case's entry point on `dev`: {name: numpy array} of everything it returns."""
    import torch
    from projectiontrainer_amd import _lib as L
    lib = L.lib()
    inp = make_inputs(c)
    rows, V = inp["rows"], c["V"]
    lg = inp["logits"].to(dev)
    hist = inp["history"].to(dev) if "history" in inp else None
    hp, hld = (hist.data_ptr(), hist.stride(0)) if hist is not None else (None, 0)
    st = L.stream_ptr(dev)
    if c["kind"] == "sample":
        fin = inp["finished"].to(dev)
        out = torch.full((rows,), SENTINEL, dtype=torch.int64, device=dev)
        n = lib.ptk_sample_next_token_workspace_bytes(rows)
        ws = torch.zeros(n, dtype=torch.uint8, device=dev)
        rc = lib.ptk_sample_next_token(lg.data_ptr(), lg.stride(0), rows, V, c["do_sample"], c["top_k"],
                                       c["temperature"], c["top_p"], 0x5eed0000 + len(c["id"]), c["step"], EOS, PAD,
                                       fin.data_ptr(), hp, hld, c["n_hist"], c["penalty"], out.data_ptr(),
                                       ws.data_ptr(), n, st)
        torch.cuda.synchronize(dev)
        return {"rc": np.array([rc], np.int32), "tok": out.cpu().numpy(), "finished": fin.cpu().numpy()}
    B, K, nc = c["batch"], c["K"], c["n_cand"]
    bs = inp["beam_scores"].to(dev)
    tok = torch.full((B, nc), SENTINEL, dtype=torch.int64, device=dev)
    bi = torch.full((B, nc), SENTINEL, dtype=torch.int32, device=dev)
    sc = torch.full((B, nc), float(SENTINEL), dtype=torch.float32, device=dev)
    pen = c["penalized_entry"]
    n = (lib.ptk_beam_candidates_penalized_workspace_bytes if pen else lib.ptk_beam_candidates_workspace_bytes)(B, K, nc)
    ws = torch.zeros(n, dtype=torch.uint8, device=dev)
    head = (lg.data_ptr(), lg.stride(0), bs.data_ptr(), B, K, V, c["do_sample"], c["top_k"], c["top_p"],
            c["temperature"], c["min_keep"], 0xbea30000 + len(c["id"]), c["step"], nc)
    tail = (tok.data_ptr(), bi.data_ptr(), sc.data_ptr(), ws.data_ptr(), n, st)
    if pen:
        rc = lib.ptk_beam_candidates_penalized(*head, hp, hld, c["n_hist"], c["penalty"], *tail)
    else:
        rc = lib.ptk_beam_candidates(*head, *tail)
    torch.cuda.synchronize(dev)
    return {"rc": np.array([rc], np.int32), "tok": tok.cpu().numpy(), "beam": bi.cpu().numpy(),
            "score_bits": sc.cpu().numpy().view(np.int32)}


def workspace_cases():
    """(name, function, arguments after the config) for the tiny, cfg2 and cfg5 presets."""
    from projectiontrainer_amd.config import PRESETS
    out = []
    for name in ("tiny", "cfg2", "cfg5"):
        cfg = PRESETS[name]
        B, T = cfg.batch_size, cfg.text_len
        Sp = (cfg.seq_len + 63) // 64 * 64
        P = cfg.num_vision_tokens
        out.append((name, cfg.text, B, T, Sp, P))
    return out


def workspace_table():
    """{name: bytes} of the four Gemma3 workspace queries per preset (they launch nothing)."""
    from projectiontrainer_amd import _lib as L
    lib = L.lib()
    tab = {}
    for name, t, B, T, Sp, P in workspace_cases():
        cc = L.Gemma3ConfigC(t.vocab_size, t.hidden_size, t.intermediate_size, t.num_hidden_layers,
                             t.num_attention_heads, t.num_key_value_heads, t.head_dim, t.sliding_window,
                             t.sliding_window_pattern, t.pad_token_id, float(t.query_pre_attn_scalar), t.rms_norm_eps)
        tab[f"ws/{name}/gemma3"] = lib.ptk_gemma3_workspace_bytes(C.byref(cc), B, T, Sp)
        tab[f"ws/{name}/train"] = lib.ptk_gemma3_train_workspace_bytes(C.byref(cc), B, T, Sp)
        tab[f"ws/{name}/generate"] = lib.ptk_gemma3_generate_workspace_bytes(C.byref(cc), B, P, 64)
        d = L.Gemma3DecodeC(3 * min(B, 4), P + 64, 128, 3, P + 64)
        tab[f"ws/{name}/decode"] = lib.ptk_gemma3_decode_workspace_bytes(C.byref(cc), C.byref(d))
    return tab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    dev = torch.device("cuda:0")
    rec = {}
    for c in cases():
        a, b = run_case(c, dev), run_case(c, dev)
        diff = [k for k in a if not np.array_equal(a[k], b[k])]
        if diff:
            sys.exit(f"{c['id']}: two runs differ in {diff}; nothing written")
        for k, v in a.items():
            rec[f"{c['id']}/{k}"] = v
        print(c["id"], "rc", int(a["rc"][0]), "tok", a["tok"].ravel()[:6].tolist())
    for k, v in workspace_table().items():
        rec[k] = np.array([v], np.int64)
    missing = REQUIRED_PATHS - set().union(*[c["paths"] for c in cases()])
    if missing:
        sys.exit(f"case list misses {sorted(missing)}")
    np.savez_compressed(args.out, **rec)
    print(f"wrote {args.out}: {len(cases())} cases, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
