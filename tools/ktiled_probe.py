"""Row-major B against its k-step-tiled copy (kernels.pack_kstep_tiles, ptk_gemm_desc.B_kt) on the persistent GEMMs
of the cfg2 step: HIP-event time per launch, the two forms alternated in one process, bit-equality checked.

  python tools/ktiled_probe.py [shape ...]          time every shape (or the named ones), ROUNDS alternations (default 5)
  python tools/ktiled_probe.py --once FORM shape     one warm-up and one launch of FORM (rowmajor | tiled) of one shape, for a
                                                     counter run: rocprofv3 --pmc TCP_TCC_READ_REQ_sum -- python tools/ktiled_probe.py --once ...
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


def main():
    args = sys.argv[1:]
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
