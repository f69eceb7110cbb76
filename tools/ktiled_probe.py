"""Row-major B against its k-step-tiled copy (kernels.pack_kstep_tiles, ptk_gemm_desc.B_kt) on the persistent GEMMs
of the cfg2 step: HIP-event time per launch, the two forms alternated in one process, bit-equality checked.

  python tools/ktiled_probe.py [shape ...]          time every shape (or the named ones), ROUNDS alternations (default 5)
  python tools/ktiled_probe.py --once FORM shape     one warm-up and one launch of FORM (rowmajor | tiled) of one shape, for a
                                                     counter run: rocprofv3 --pmc TCP_TCC_READ_REQ_sum -- python tools/ktiled_probe.py --once ...
  python tools/ktiled_probe.py --a [shape ...]      the A side: row-major A against a k-step-tiled A (ptk_gemm_desc.A_kt,
                                                     packed on the device by the same kernel), B tiled in both forms;
                                                     default shapes g_dgu_dx and g_down.  --once takes the forms
                                                     a-rowmajor | a-tiled likewise
  python tools/ktiled_probe.py --p [shape ...]      the producers g_gu_geglu and g_dh_geglu_bwd: row-major outputs against
                                                     tiled C (C_kt) and tiled C + GEGLU factors (aux_kt / aux_in_kt), B
                                                     tiled in every form; equal = the tiled outputs are the pack kernel's
                                                     image of the row-major ones
Each line: the family the planner chose, min and max us per form over the rounds, and the ratio of the minima."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from projectiontrainer_amd import kernels as K, _lib as L  # noqa: E402

dev = torch.device("cuda:0")
M1, MS = 32 * 704, 32 * 576
SHAPES = {  # name: M, N, K, act
    "g_gu_geglu": (M1, 13824, 1152, L.ACT_GEGLU),
    "g_down": (M1, 1152, 6912, L.ACT_NONE),
    "g_dgu_dx": (M1, 1152, 13824, L.ACT_NONE),
    "g_dh_geglu_bwd": (M1, 6912, 1152, L.ACT_GEGLU_BWD),
    "g_qkv": (M1, 1536, 1152, L.ACT_NONE),
    "g_o": (M1, 1152, 1024, L.ACT_NONE),
    "g_dqkv": (M1, 1152, 1536, L.ACT_NONE),
    "sig_qkv": (MS, 3072, 1024, L.ACT_NONE),
    "sig_fc1": (MS, 4096, 1024, L.ACT_GELU_TANH),
    "sig_fc2": (MS, 1024, 4096, L.ACT_NONE),
}


def setup(m, n, k, act):
    A = torch.randn(m, k, device=dev).to(torch.bfloat16)
    B = (torch.randn(n, k, device=dev) * 0.05).to(torch.bfloat16)
    kw = {}
    if act == L.ACT_GEGLU:
        kw = dict(aux=torch.empty(m, n // 2, dtype=torch.bfloat16, device=dev),
                  aux2=torch.empty(m, n // 2, dtype=torch.bfloat16, device=dev))
    elif act == L.ACT_GEGLU_BWD:
        kw = dict(aux_in=torch.randn(m, n, device=dev).to(torch.bfloat16),
                  aux_in2=torch.randn(m, n, device=dev).to(torch.bfloat16))
    return A, B, kw


def timed(A, B, Bkt, kw, act, C, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        K.gemm(A, B, C=C, act=act, B_kt=Bkt, **kw)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


A_SHAPES = ("g_dgu_dx", "g_down")


def timed_a(A, B, Bkt, a_kt, C, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        K.gemm(A, B, C=C, B_kt=Bkt, A_kt=a_kt)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def main_a(names, rounds):
    for name in (names or A_SHAPES):
        m, n, k, act = SHAPES[name]
        assert act == L.ACT_NONE, "the tiled-A variant has the plain epilogue only"
        A, B, _ = setup(m, n, k, act)
        Bkt, Akt = K.pack_kstep_tiles(B), K.pack_kstep_tiles(A)
        L.gemm_path_counts(reset=True)
        C0 = K.gemm(A, B, B_kt=Bkt)
        fam = sorted({p for p, _ in L.gemm_path_counts(reset=True)})
        L.gemm_ktiled_counts(reset=True)
        C1 = K.gemm(Akt, B, B_kt=Bkt, A_kt=True)
        torch.cuda.synchronize()
        assert L.gemm_ktiled_counts(reset=True)[0] == 1
        reps = max(3, min(50, int(2e12 / (2.0 * m * n * k))))
        res = {"a_rowmajor": [], "a_tiled": []}
        Cs = torch.empty_like(C0)
        for _ in range(rounds):
            for form, a, flag in (("a_rowmajor", A, False), ("a_tiled", Akt, True)):
                timed_a(a, B, Bkt, flag, Cs, 1)
                res[form].append(timed_a(a, B, Bkt, flag, Cs, reps))
        out = {"name": name, "M": m, "N": n, "K": k, "family": fam, "equal": bool(torch.equal(C0, C1))}
        for form, v in res.items():
            out[form + "_us"] = [round(min(v), 1), round(max(v), 1)]
        out["a_tiled/a_rowmajor"] = round(min(res["a_tiled"]) / min(res["a_rowmajor"]), 4)
        print(json.dumps(out), flush=True)
        del A, B, Bkt, Akt, C0, C1, Cs
        torch.cuda.empty_cache()


P_SHAPES = ("g_gu_geglu", "g_dh_geglu_bwd")


def main_p(names, rounds):
    for name in (names or P_SHAPES):
        m, n, k, act = SHAPES[name]
        A, B, kw = setup(m, n, k, act)
        Bkt = K.pack_kstep_tiles(B)
        glu = act == L.ACT_GEGLU
        kw_t = dict(kw) if glu else {q: K.pack_kstep_tiles(v) for q, v in kw.items()}   # the factors read tiled
        fac = dict(aux_kt=True) if glu else dict(aux_in_kt=True)
        forms = {"rowmajor": (kw, {}), "tiled_c": (kw, dict(C_kt=True)), "tiled_c_fac": (kw_t, dict(C_kt=True, **fac))}
        L.gemm_path_counts(reset=True)
        outs = {}
        for form, (k1, k2) in forms.items():
            C = K.gemm(A, B, act=act, B_kt=Bkt, **k1, **k2)
            outs[form] = [C] + ([k1["aux"].clone(), k1["aux2"].clone()] if glu else [])
        fam = sorted({p for p, _ in L.gemm_path_counts(reset=True)})
        torch.cuda.synchronize()
        eq = torch.equal(K.pack_kstep_tiles(outs["rowmajor"][0]), outs["tiled_c"][0])
        eq = eq and all(torch.equal(K.pack_kstep_tiles(r), t) for r, t in zip(outs["rowmajor"], outs["tiled_c_fac"]))
        eq = eq and all(torch.equal(r, t) for r, t in zip(outs["rowmajor"][1:], outs["tiled_c"][1:]))
        reps = max(3, min(50, int(2e12 / (2.0 * m * n * k))))
        res = {f: [] for f in forms}
        C0 = outs["rowmajor"][0]
        for _ in range(rounds):
            for form, (k1, k2) in forms.items():
                for r in (1, reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _i in range(r):
                        K.gemm(A, B, C=C0, act=act, B_kt=Bkt, **k1, **k2)
                    e1.record()
                    torch.cuda.synchronize()
                res[form].append(e0.elapsed_time(e1) / reps * 1e3)
        out = {"name": name, "M": m, "N": n, "K": k, "family": fam, "equal": bool(eq)}
        for form, v in res.items():
            out[form + "_us"] = [round(min(v), 1), round(max(v), 1)]
        for form in ("tiled_c", "tiled_c_fac"):
            out[form + "/rowmajor"] = round(min(res[form]) / min(res["rowmajor"]), 4)
        print(json.dumps(out), flush=True)
        del A, B, Bkt, kw, kw_t, outs, C0
        torch.cuda.empty_cache()


def main():
    args = sys.argv[1:]
    if args and args[0] == "--p":
        return main_p(args[1:], int(os.environ.get("ROUNDS", "5")))
    if args and args[0] == "--once" and args[1].startswith("a-"):
        m, n, k, act = SHAPES[args[2]]
        A, B, _ = setup(m, n, k, act)
        Bkt, tiled = K.pack_kstep_tiles(B), args[1] == "a-tiled"
        if tiled:
            A = K.pack_kstep_tiles(A)
        C = K.gemm(A, B, B_kt=Bkt, A_kt=tiled)
        K.gemm(A, B, C=C, B_kt=Bkt, A_kt=tiled)
        torch.cuda.synchronize()
        return
    if args and args[0] == "--a":
        return main_a(args[1:], int(os.environ.get("ROUNDS", "5")))
    if args and args[0] == "--once":
        form, name = args[1], args[2]
        m, n, k, act = SHAPES[name]
        A, B, kw = setup(m, n, k, act)
        Bkt = K.pack_kstep_tiles(B) if form == "tiled" else None
        C = K.gemm(A, B, act=act, B_kt=Bkt, **kw)
        K.gemm(A, B, C=C, act=act, B_kt=Bkt, **kw)
        torch.cuda.synchronize()
        return
    rounds = int(os.environ.get("ROUNDS", "5"))
    for name in (args or SHAPES):
        m, n, k, act = SHAPES[name]
        A, B, kw = setup(m, n, k, act)
        Bkt = K.pack_kstep_tiles(B)
        L.gemm_path_counts(reset=True)
        C0 = K.gemm(A, B, act=act, **kw)
        fam = sorted({p for p, _ in L.gemm_path_counts(reset=True)})
        C1 = K.gemm(A, B, act=act, B_kt=Bkt, **kw)
        torch.cuda.synchronize()
        reps = max(3, min(50, int(2e12 / (2.0 * m * n * k))))
        res = {"rowmajor": [], "tiled": []}
        for _ in range(rounds):
            for form, kt in (("rowmajor", None), ("tiled", Bkt)):
                timed(A, B, kt, kw, act, C0, 1)
                res[form].append(timed(A, B, kt, kw, act, C0, reps))
        out = {"name": name, "M": m, "N": n, "K": k, "family": fam, "equal": bool(torch.equal(C0, C1))}
        for form, v in res.items():
            out[form + "_us"] = [round(min(v), 1), round(max(v), 1)]
        out["tiled/rowmajor"] = round(min(res["tiled"]) / min(res["rowmajor"]), 4)
        print(json.dumps(out), flush=True)
        del A, B, Bkt, C0, C1, kw
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
