#!/usr/bin/env python
"""Record what every GEMM shape of the benchmarked steps dispatches to, from any commit's libptk.so, without a GPU.

    python tools/gemm_dispatch_table.py --out tests/data/gemm_dispatch_parent.json      (PTK_LIB=.. for another build)

With no device visible ptk_gemm fails at the launch, after the dispatch census (ptk_gemm_path_counts) has counted the
kernel family and with the CU count at its 256 fallback; ptk_gemm_tail_split gives the stream-K split.  Only those
three entry points are used, so the script runs against a library that predates ptk_gemm_plan.  The script hides
every GPU from the process before it loads the library and refuses to run if one is still visible: the descriptors
carry placeholder pointers and must never reach a device.

What the census cannot show comes from two text files, one value line per row in the order of --dump-shapes FILE
(which writes FILE.tile, "M N act out" per row, and FILE.split, "M N K out ldc resid16 part_floats tail" per split row):
  --tile-heights  the 8-wave kernel's tile rows for the rows whose path is "p8" under force mode 0; under force modes
                  512 / 1024 / 4096 a "p8" row has 224 / 192 / 160 rows by the mode's definition (include/ptk.h)
  --splits        gemm_split's decision for the split rows: "slices kc rem tail_ws" (kc 0: unsplit)
Without the files the library's own ptk_gemm_plan / ptk_gemm_split_plan fill those columns (a library that has them).
For a library that predates them (the committed table's parent) two small C++ programs, built in a scratch directory
against that commit's csrc/ (SRC) and libptk.so (LIB), printed the files:
  tile heights: main() reads "M N act out" lines, sets GemmArgs::M / N and prints ptk::p8_tile_height(a, act, out);
      hipcc -std=c++17 --offload-arch=gfx950 -ISRC -x hip -c tile.cpp && hipcc tile.o -o tile -LLIB -lptk -Wl,-rpath,LIB
  splits: a file that #includes SRC/models.cpp (gemm_split is in its anonymous namespace) and defines
      ptk::launch_gemm (logs the first call's batch and K, whether tail_ws is the `part` pointer, a second call's K;
      returns 0) and ptk::launch_splitk_reduce (logs that a split happened) ahead of the library's; main() reads the
      split lines, builds the GemmArgs (identity strides; resid16: bf16_linear + resid16 == C, ld N; tail: a tail_ws
      standing for the model-level scope), calls gemm_split(a, out, part, part_floats, nullptr) and prints
      "1 0 0 tail_ws" when no reduce ran, else "first_batch first_K second_K 0"; built and linked the same way.
tests/test_gemm_plan.py pins ptk_gemm_plan / ptk_gemm_split_plan against the committed table.
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from projectiontrainer_amd import _lib as L          # noqa: E402
from projectiontrainer_amd.config import PRESETS     # noqa: E402

NONE, TANH, ERF, GEGLU, ERF_BWD, GEGLU_BWD = range(6)
BF16, F32, F32_BFR = range(3)
FORCE_MODES = (0, 1, 2, 4, 8, 32, 512, 1024, 4096)
LM_SPLITK, LM_KSLICES = 8, 16      # csrc/models.cpp


def gemm_desc_from_row(row):
    """GemmDesc of one table row (also used by tests/test_gemm_plan.py): the shape, strides, epilogue operand set,
    row maps and tail scratch as the planner sees them, with placeholder 16-B-aligned pointers."""
    d = L.GemmDesc()
    d.A, d.B, d.C = 0x10000000, 0x20000000, 0x30000000
    d.M, d.N, d.K = row["M"], row["N"], row["K"]
    d.lda, d.ldb = row.get("lda", d.K), row.get("ldb", d.K)
    d.ldc = row.get("ldc", d.N)
    d.batch, d.batch_inner = row.get("batch", 1), 1
    d.sA0, d.sA1, d.sB0, d.sB1, d.sC0, d.sC1 = row.get("strides", (0,) * 6)
    d.alpha, d.act, d.out = row.get("alpha", 1.0), row["act"], row["out"]
    for i, name in enumerate(("bias", "rowadd", "resid", "resid16", "aux", "aux2", "aux_in", "aux_in2")):
        if name in row.get("ops", ()):
            setattr(d, name, 0x40000000 + 0x1000000 * i)
    d.rowadd_period, d.ld_rowadd = row.get("rowadd_period", 1), row.get("ld_rowadd", 0)
    d.ld_resid, d.ld_resid16 = row.get("ld_resid", 0), row.get("ld_resid16", 0)
    d.ld_aux, d.ld_aux_in = row.get("ld_aux", 0), row.get("ld_aux_in", 0)
    d.amap, d.cmap = L.RowMap(*row.get("amap", (0,) * 4)), L.RowMap(*row.get("cmap", (0,) * 4))
    d.bf16_linear = row.get("bf16_linear", 0)
    d.tail_ws = 0x50000000 if row.get("tail") else None
    return d


def row(label, M, N, K, act=NONE, out=BF16, **kw):
    return dict(label=label, M=M, N=N, K=K, act=act, out=out, **kw)


def step_rows(name, cfg, B, train):
    """The GEMMs one step launches through launch_gemm (ptk_siglip_fwd, the projector, gemma_run, weight_grad's
    transpose path), each with the tail scratch its model-level call lends; the GEMMs gemm_split routes come back
    in split[] as well (their unsplit form is the row here)."""
    v, t = cfg.vision, cfg.text
    tag = f"{name}.bs{B}"
    rows, split = [], []
    # SigLIP forward
    Ms, D, I, Kp = B * v.num_patches, v.hidden_size, v.intermediate_size, v.patch_dim
    res = dict(ops=["bias", "resid16"], bf16_linear=1, ld_resid16=D, tail=True)
    rows += [row(f"{tag}.siglip.patch", Ms, D, Kp, ops=["bias", "rowadd"], bf16_linear=1, rowadd_period=v.num_patches,
                 ld_rowadd=D, tail=True),
             row(f"{tag}.siglip.qkv", Ms, 3 * D, D, ops=["bias"], tail=True),
             row(f"{tag}.siglip.o", Ms, D, D, **res),
             row(f"{tag}.siglip.fc1", Ms, I, D, act=TANH, ops=["bias"], tail=True),
             row(f"{tag}.siglip.fc2", Ms, D, I, **res)]
    # projector forward / backward (the weight grads' transpose path: PTK_WGRAD_TN=0)
    Dv, Ip, H = D, D * cfg.expansion_factor, t.hidden_size
    Sp = (cfg.seq_len + 63) // 64 * 64
    rows += [row(f"{tag}.proj.fc1", Ms, Ip, Dv, act=ERF, ops=["bias", "aux"], ld_aux=Ip, tail=True),
             row(f"{tag}.proj.fc2", Ms, H, Ip, out=F32_BFR, ops=["bias"], cmap=(v.num_patches, 1, Sp, -1), tail=True)]
    if not train:
        Rp = (Ms + 63) // 64 * 64
        rows += [row(f"{tag}.proj.dA", Ms, Ip, H, act=ERF_BWD, ops=["aux_in"], ld_aux_in=Ip, tail=True),
                 row(f"{tag}.proj.dW2", H, Ip, Rp, out=F32, tail=True),
                 row(f"{tag}.proj.dW1", Ip, Dv, Rp, out=F32, tail=True)]
    # Gemma3 forward + loss + backward
    I, Dh, Hq, Hkv, V = t.intermediate_size, t.head_dim, t.num_attention_heads, t.num_key_value_heads, t.vocab_size
    G, Dq, Dqkv = Hq // Hkv, Hq * Dh, (Hq + 2 * Hkv) * Dh
    M, lo = B * Sp, cfg.question_len
    Tl = cfg.text_len - lo
    R = B * Tl
    lossmap = (Tl, 0, Sp, cfg.num_vision_tokens - 1 + lo)

    def routed(label, m, n, k, **kw):
        r = row(f"{tag}.{label}", m, n, k, tail=True, **kw)
        rows.append(r)
        split.append(r)

    routed("gemma.qkv", M, Dqkv, H)
    routed("gemma.o", M, H, Dq)
    rows.append(row(f"{tag}.gemma.gate_up", M, 2 * I, H, act=GEGLU, ldc=I, ops=["aux", "aux2"], ld_aux=I, tail=True))
    routed("gemma.down", M, H, I)
    rows += [row(f"{tag}.gemma.last.gate_up", R, 2 * I, H, act=GEGLU, ldc=I, ops=["aux", "aux2"], ld_aux=I,
                 amap=lossmap, tail=True),
             row(f"{tag}.gemma.last.down", R, H, I, cmap=lossmap, tail=True),
             row(f"{tag}.gemma.lm_head", R, V, H, tail=True)]
    if not (R % 256 == 0 and V % (64 * LM_KSLICES) == 0):
        kc = V // (64 * LM_SPLITK) * 64
        rows.append(row(f"{tag}.gemma.lm_head_dx", R, H, kc, out=F32, lda=V, ldb=V, batch=LM_SPLITK,
                        strides=(kc, 0, kc, 0, R * H, 0), tail=True))
        if V - LM_SPLITK * kc:
            rows.append(row(f"{tag}.gemma.lm_head_dx.rem", R, H, V - LM_SPLITK * kc, out=F32, lda=V, ldb=V, tail=True))
    rows.append(row(f"{tag}.gemma.dh_geglu_bwd", M, I, H, act=GEGLU_BWD, ldc=2 * I, ops=["aux_in", "aux_in2"],
                    ld_aux_in=I, tail=True))
    routed("gemma.dgu_dx", M, H, 2 * I)
    rows += [row(f"{tag}.gemma.dO", M, G * Dh, H, batch=Hkv, cmap=(Sp, 0, Hkv * Sp, 0),
                 strides=(0, 0, G * Dh * H, 0, Sp * G * Dh, 0), tail=True)]
    routed("gemma.dqkv_dx", M, H, Dqkv)
    rows += [row(f"{tag}.gemma.last.dh", R, I, H, amap=lossmap, tail=True),
             row(f"{tag}.gemma.last.dgu_dx", R, H, 2 * I, cmap=lossmap, tail=True)]
    if train:   # weight grads on the transpose path: [Ny, Nx] (+)= over Kp token rows, the bf16 accumulate epilogue
        def wgrad(label, Ny, Nx, rows_):
            Kp_ = (rows_ + 63) // 64 * 64
            routed(label, Ny, Nx, Kp_, ops=["resid16"], bf16_linear=1, ld_resid16=Nx)
        wgrad("gemma.dW_qkv", Dqkv, H, M)
        wgrad("gemma.dW_o", H, Dq, M)
        wgrad("gemma.dW_down", H, I, M)
        wgrad("gemma.dW_gate_up", 2 * I, H, M)
        wgrad("gemma.last.dW_down", H, I, R)
        wgrad("gemma.last.dW_gate_up", 2 * I, H, R)
    return rows, split


def boundary_rows():
    rows = []
    for M in (4095, 4096):   # the persistent kernels' M gate
        rows += [row(f"edge.M{M}.single_round", M, 2048, 1024), row(f"edge.M{M}.geglu", M, 13824, 1152, act=GEGLU, ldc=6912)]
    for K in (2048, 2112):   # p8-over-w4
        rows += [row(f"edge.K{K}.plain", 16384, 4096, K), row(f"edge.K{K}.plain_f32", 16384, 4096, K, out=F32),
                 row(f"edge.K{K}.tanh", 16384, 4096, K, act=TANH),
                 row(f"edge.K{K}.erf", 16384, 10240, K, act=ERF, ops=["bias", "aux"], ld_aux=10240),
                 row(f"edge.K{K}.n1536", 14336, 1536, K)]
    for K in (4032, 4096, 4160, 4224):   # the tail's K gate and its odd K-tile counts; staggered-big
        rows += [row(f"edge.K{K}.tail", 14336, 1152, K, tail=True), row(f"edge.K{K}.tail_f32", 14336, 1152, K, out=F32, tail=True),
                 row(f"edge.K{K}.no_scratch", 14336, 1152, K), row(f"edge.K{K}.big", 2048, 8192, K)]
    for K in (8192, 8256):   # w4 and single-round K limits
        rows += [row(f"edge.K{K}.w4", 16384, 4096, K), row(f"edge.K{K}.single_round", 4096, 2048, K),
                 row(f"edge.K{K}.single_round_tail", 4096, 2048, K, tail=True)]
    for K in (12224, 12288):   # long-K plain projections on the 8-wave kernel
        rows += [row(f"edge.K{K}.n2048", 16384, 2048, K), row(f"edge.K{K}.n2304", 16384, 2304, K),
                 row(f"edge.K{K}.n1152_tail", 22528, 1152, K, tail=True)]
    for N in (1024, 1152, 1536):   # Gemma3's / SigLIP's narrow projections
        for K in (1152, 2048, 6912):
            rows += [row(f"edge.N{N}.K{K}", 22528, N, K), row(f"edge.N{N}.K{K}.tail", 22528, N, K, tail=True)]
    for mt in list(range(52, 60)) + list(range(100, 112, 2)):   # round fill around 0.65 (N 1536: 6 tile columns)
        rows.append(row(f"edge.fill65.mt{mt}", 256 * mt, 1536, 1152))
    for mt in range(16, 27):   # round fill around 0.8 (40 tile columns; GELU-erf has no short tiles)
        rows += [row(f"edge.fill80.erf.mt{mt}", 256 * mt, 10240, 1024, act=ERF, ops=["bias", "aux"], ld_aux=10240),
                 row(f"edge.fill80.plain.mt{mt}", 256 * mt, 10240, 1024)]
    rows += [row("edge.tiles256", 65536, 256, 1024), row("edge.tiles257", 65792, 256, 1024),
             row("edge.tiles255", 4352, 3840, 1024), row("edge.tiles272", 4352, 4096, 1024)]
    for N in (255, 256, 16384, 16392):   # the tail's N gate
        rows.append(row(f"edge.tailN{N}", 4096 if N > 256 else 65536, N // 8 * 8, 4096, tail=True))
    for M in (1023, 1024):   # the tail's M gate (a single tile column, 4 tiles)
        rows.append(row(f"edge.tailM{M}", M, 256, 8192, tail=True))
    for f in FORCE_MODES:   # every force mode on a plain and a GELU-tanh shape, with and without tail scratch
        rows += [row(f"force{f}.plain", 22528, 1152, 6912, force=f), row(f"force{f}.plain_tail", 22528, 1152, 6912, force=f, tail=True),
                 row(f"force{f}.tanh", 18432, 4096, 1024, act=TANH, ops=["bias"], force=f),
                 row(f"force{f}.small", 520, 1152, 6912, force=f)]
    rows += [row("edge.batch2", 22528, 1152, 1152, batch=2, strides=(0, 0, 1152 * 1152, 0, 22528 * 1152, 0)),
             row("edge.batch2_geglu", 22528, 13824, 1152, act=GEGLU, ldc=6912, batch=2),
             row("edge.ldc_unaligned", 22528, 1152, 6912, ldc=1156), row("edge.ldc_unaligned_tail", 14336, 1152, 6912, ldc=1156, tail=True),
             row("edge.alpha", 22528, 1152, 6912, alpha=0.5), row("edge.alpha_geglu", 22528, 13824, 1152, act=GEGLU, ldc=6912, alpha=0.5),
             row("edge.amap_gather", 16384, 4096, 1024, amap=(128, 0, 704, 575)),
             row("edge.resid_f32", 22528, 1152, 6912, out=F32, ops=["resid"], ld_resid=1152)]
    return rows


def all_rows():
    rows, split = [], []
    for name, B, train in (("cfg2", 32, False), ("cfg2", 30, False), ("cfg5", 16, False), ("cfg5", 8, False),
                           ("cfg4", 16, True), ("cfg4", 8, True), ("cfg1", 2, False)):
        r, s = step_rows(name, PRESETS[name], B, train)
        rows += r
        split += s
        if name in ("cfg4", "cfg1"):   # and without a model-level tail scope: gemm_split lends its own scratch
            split += [dict(x, tail=False, label=x["label"] + ".no_scope") for x in s]
    rows += boundary_rows()
    # K splits with an odd K-tile count: one full slice of depth kc plus a remainder slice
    big = sk_floats(PRESETS["cfg4"], 16, True)
    for M, K in ((14336, 4160), (14336, 7104), (520, 576), (520, 704), (520, 6976)):
        for tail in (True, False):
            split.append(row(f"edge.split.M{M}.K{K}" + ("" if tail else ".no_scope"), M, 1152, K, tail=tail, part_floats=big))

    def key(r):
        return json.dumps({k: v for k, v in r.items() if k != "label"}, sort_keys=True)

    def dedup(rs):
        seen, out = {}, []
        for r in rs:
            if key(r) in seen:
                seen[key(r)]["label"] += "," + r["label"]
            else:
                seen[key(r)] = r
                out.append(r)
        return out
    return dedup(rows), dedup([dict(r) for r in split])


def sk_floats(cfg, B, train):
    """GemmaWs::sk_floats (csrc/models.cpp gemma_layout) at 256 CUs: the fp32 scratch gemm_split may use"""
    t = cfg.text
    Sp = (cfg.seq_len + 63) // 64 * 64
    M, H, I = B * Sp, t.hidden_size, t.intermediate_size
    Dqkv = (t.num_attention_heads + 2 * t.num_key_value_heads) * t.head_dim
    n = max(2 * M * H, 2 * 2 * I * H, 4 * max(Dqkv, H) * H)
    if train:
        n = max(n, t.vocab_size * H)
    slab = 256 * 2 * 8 * 128 * 64
    n = max(n, (16384 + slab * 4) // 4 + 64)
    return max(n, slab) if train else n


def no_device_visible():
    try:
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        return True
    n = C.c_int(0)
    return hip.hipGetDeviceCount(C.byref(n)) != 0 or n.value == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--dump-shapes", help="write the rows as text for the C++ recorders: <file>.tile and <file>.split")
    ap.add_argument("--tile-heights")
    ap.add_argument("--splits")
    args = ap.parse_args()
    rows, split = all_rows()
    cfg_of = {f"{n}.bs{b}": (PRESETS[n], b, tr) for n, b, tr in (("cfg2", 32, 0), ("cfg2", 30, 0), ("cfg5", 16, 0),
                                                               ("cfg5", 8, 0), ("cfg4", 16, 1), ("cfg4", 8, 1), ("cfg1", 2, 0))}
    for s in split:
        if "part_floats" in s:
            continue
        c, b, tr = cfg_of[".".join(s["label"].split(",")[0].split(".")[:2])]
        s["part_floats"] = sk_floats(c, b, bool(tr))
    if args.dump_shapes:
        with open(args.dump_shapes + ".tile", "w") as f:
            for r in rows:
                f.write(f"{r['M']} {r['N']} {r['act']} {r['out']}\n")
        with open(args.dump_shapes + ".split", "w") as f:
            for s in split:
                f.write(f"{s['M']} {s['N']} {s['K']} {s['out']} {s.get('ldc', s['N'])} {int('resid16' in s.get('ops', ()))} "
                        f"{s['part_floats']} {int(bool(s.get('tail')))}\n")
    if not args.out:
        return
    for v in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES"):   # before the first HIP call of this process
        os.environ[v] = "-1"
    if not no_device_visible():
        sys.exit("a GPU is visible: this script launches with placeholder pointers and only runs without a device")
    lib = L.lib()
    heights = [int(x) for x in open(args.tile_heights).read().split()] if args.tile_heights else [None] * len(rows)
    if not args.tile_heights:   # the library's own planner
        for i, r in enumerate(rows):
            tm = C.c_int(0)
            L.check(lib.ptk_gemm_plan(gemm_desc_from_row(r), 256, None, C.byref(tm), None), "ptk_gemm_plan")
            heights[i] = tm.value
    for r, h in zip(rows, heights):
        L.check(lib.ptk_gemm_force_small_tiles(r.get("force", 0)), "force")
        d = gemm_desc_from_row(r)
        L.gemm_path_counts(reset=True)
        lib.ptk_gemm(d, None)   # fails at the launch (no device), after the census
        counts = L.gemm_path_counts(reset=True)
        assert len(counts) == 1 and sum(counts.values()) == 1, (r, counts)
        (path, act), = counts.keys()
        assert act == r["act"]
        r["path"] = path
        r["tail_split_raw"] = lib.ptk_gemm_tail_split(d)   # (without launch_gemm's gates)
        r["tile_rows"] = None
        if path == "p8":
            r["tile_rows"] = {0: h, 32: 256, 512: 224, 1024: 192, 4096: 160}[r.get("force", 0)]
    L.check(lib.ptk_gemm_force_small_tiles(0), "force")
    if args.splits:
        vals = [[int(x) for x in ln.split()] for ln in open(args.splits) if ln.strip()]
        assert len(vals) == len(split)
        for s, (slices, kc, rem, tail_ws) in zip(split, vals):
            s.update(slices=slices, kc=kc, rem=rem, tail_ws=tail_ws)
    else:
        for s in split:
            o = [C.c_int(0) for _ in range(4)]
            L.check(lib.ptk_gemm_split_plan(gemm_desc_from_row(s), 256, s["part_floats"], *[C.byref(x) for x in o]), "split_plan")
            s.update(slices=o[0].value, kc=o[1].value, rem=o[2].value, tail_ws=o[3].value)
    with open(args.out, "w") as f:
        f.write('{"ncu": 256,\n "rows": [\n  ' + ",\n  ".join(json.dumps(r) for r in rows) + '\n ],\n "split_rows": [\n  ' +
                ",\n  ".join(json.dumps(s) for s in split) + "\n ]}\n")
    print(len(rows), "rows,", len(split), "split rows ->", args.out)


if __name__ == "__main__":
    main()
