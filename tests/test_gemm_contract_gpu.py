"""Every GEMM kernel family against the descriptor's contract in fp64 (tests/gemm_ref.py): row maps on A and C, the
additive inputs, every output mode, padded leading dimensions, ragged M and N, the six activations, batched launches,
each under every force mode, on operands whose sums are exact in fp32 in any order.  ACT_NONE, the stored
pre-activations and the GEGLU backward are compared bit for bit; the transcendental epilogues under the two
conditions of gemm_ref (REL_TOL |ref| + floor on every element, at most NEQ_CAP of them not bit-equal).  Every
output buffer sits between guard rows and has guard-filled padding columns, every input is NaN outside what the
contract reads, and the family that ran is held to the pinned table (tests/data/gemm_contract_plan.json).

PTK_GEMM_CONTRACT_REPORT=<file>: the last test also writes its per-family tally there (cases, bit-exact cases, the
largest not-bit-equal share of each transcendental output)."""
import json
import os

import pytest
import torch

from tests import gemm_ref as G

pytestmark = pytest.mark.gpu
TALLY = {}      # family -> {"cases": n, "exact": n, "neq": {output: largest share}}


@pytest.fixture(scope="module")
def env(gpu):
    from projectiontrainer_amd import _lib as L
    from projectiontrainer_amd import kernels as Kn
    L.gemm_path_counts(reset=True)
    return L, Kn, L.lib(), G.load_plan_table(), gpu


def _launch(env, mode, fn):
    """fn() under force mode `mode`; returns the census of what ran."""
    L, _, lib = env[:3]
    L.gemm_path_counts(reset=True)
    L.check(lib.ptk_gemm_force_small_tiles(mode), "force")
    try:
        fn()
    finally:
        lib.ptk_gemm_force_small_tiles(0)
    return L.gemm_path_counts(reset=True)


def _tally(fam, act, stats):
    t = TALLY.setdefault(fam, {"cases": 0, "exact": 0, "neq": {}})
    t["cases"] += 1
    t["exact"] += all(neq == 0 for _, neq in stats.values())
    if act not in G.EXACT_ACTS:
        for name, (n, neq) in stats.items():
            if name == "aux" and act in (G.ACT_GELU_TANH, G.ACT_GELU_ERF):
                continue
            key = f"{G.ACT_NAMES[act]}.{name}"
            t["neq"][key] = max(t["neq"].get(key, 0.0), neq / n)


def _run_case(env, c, M, modes):
    L, Kn, lib, table, dev = env
    b = G.build(c, M, dev)
    r = G.ref(b.A, b.B, **b.kw)
    failed = []
    for mode in modes:
        G.restore(b)
        fam = table[c["id"]][str(M)][str(mode)]
        ran = _launch(env, mode, lambda: Kn.gemm(b.A, b.B, **b.kw))
        assert ran == {(fam.split("@")[0], c["act"]): 1}, (c["id"], M, mode, ran, fam)
        stats, bad = G.check(b, r, f"{c['id']} M={M} mode={mode} {fam}")
        _tally(fam, c["act"], stats)
        failed += bad
    return failed


@pytest.mark.parametrize("cid", [c["id"] for c in G.CASES])
def test_case(env, cid):
    c = G.CASE_BY_ID[cid]
    failed = [f for M in G.MS for f in _run_case(env, c, M, G.MODES)]
    assert not failed, "\n".join(failed)


def test_second_tile_round_of_the_persistent_families(env):
    """More tiles than compute units: a workgroup's second tile derives its row state (group cmap, fp32 resid, bias)
    again."""
    dev = env[4]
    c, M = G.ROUND2, G.ROUND2["M"]
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    assert -(-M // 256) * -(-c["N"] // 256) > ncu, ncu
    failed = _run_case(env, c, M, G.ROUND2_MODES)
    assert not failed, "\n".join(failed)


def _batched(env, *, M, N, K, nz, zin, a_rows, b_rows, c_rows, ldc, strides, cmap, alpha, a_of, b_of):
    """One batched launch (always the batched 128x128 kernel) against ref(): A / B blocks placed by a_of(z) / b_of(z)
    (first row of batch z's block) into NaN buffers, C guard-filled."""
    L, Kn, lib, _, dev = env
    lda = ldb = K + 8
    A = G.nan_buffer(a_rows, lda, torch.bfloat16, dev)
    B = G.nan_buffer(b_rows, ldb, torch.bfloat16, dev)
    for z in sorted({a_of(z) for z in range(nz)}):
        A[z:z + M, :K] = G.dyadic((M, K), -2, 2, 0, 7000 + z).to(dev)
    for z in sorted({b_of(z) for z in range(nz)}):
        B[z:z + N, :K] = G.dyadic((N, K), -4, 4, 6, 8000 + z).to(dev)
    full = G.guard_fill(torch.empty((G.FRONT + c_rows + G.BACK, ldc), dtype=torch.bfloat16, device=dev))
    init, view = full.clone(), full[G.FRONT:]
    kw = dict(C=view, M=M, N=N, K=K, alpha=alpha, batch=nz, batch_inner=zin, strides=strides, cmap=cmap)
    r = G.ref(A, B, **kw)
    assert int(r.written["C"].sum()) == nz * M * N            # (the batches' outputs do not overlap)
    for mode in G.MODES:
        full.copy_(init)
        ran = _launch(env, mode, lambda: Kn.gemm(A, B, **kw))
        assert ran == {("nt128b", G.ACT_NONE): 1}, (mode, ran)
        n, neq, bad, worst, stray, lost = G.measure(full, init, view, r, "C")
        print(f"batched mode={mode}: written {n} not-bit-equal {neq} stray {stray} guard-lost {lost}")
        assert (neq, stray, lost) == (0, 0, 0), (mode, n, neq, stray, lost)
        _tally("nt128b", G.ACT_NONE, {"C": (n, neq)})


def test_batched_all_six_strides(env):
    """batch 6 = 3 x 2 with every stride set and distinct, ragged M and N, alpha 0.125, ldc wider than N."""
    M, N, K = 150, 200, 128
    lda, ldc = K + 8, N + 8
    ra1, ra0 = M + 8, 2 * (M + 8) + 16          # rows between the A blocks of (z0, z1 + 1) / (z0 + 1, z1)
    rb1, rb0 = N + 8, 2 * (N + 8) + 24
    rc1, rc0 = M + 4, 2 * (M + 4) + 3
    zz = lambda z: divmod(z, 2)
    _batched(env, M=M, N=N, K=K, nz=6, zin=2, a_rows=3 * ra0, b_rows=3 * rb0, c_rows=3 * rc0, ldc=ldc,
             strides=(ra0 * lda, ra1 * lda, rb0 * lda, rb1 * lda, rc0 * ldc, rc1 * ldc), cmap=(0, 0, 0, 0), alpha=0.125,
             a_of=lambda z: zz(z)[0] * ra0 + zz(z)[1] * ra1, b_of=lambda z: zz(z)[0] * rb0 + zz(z)[1] * rb1)


def test_batched_dO_form(env):
    """The dO GEMM of the Gemma3 backward: one A for every kv head, sB0 / sC0 per head, the result scattered into the
    [batch, kv head, position, group x dim] layout through cmap = (Sp, 0, Hkv Sp, 0)."""
    Sp, Hkv, GD, H, nb = 96, 4, 136, 128, 3
    M, ldc = nb * Sp - 20, GD + 8               # (the last sequence is cut short: ragged M)
    _batched(env, M=M, N=GD, K=H, nz=Hkv, zin=1, a_rows=M + 8, b_rows=Hkv * GD + 8, c_rows=nb * Hkv * Sp, ldc=ldc,
             strides=(0, 0, GD * (H + 8), 0, Sp * ldc, 0), cmap=(Sp, 0, Hkv * Sp, 0), alpha=0.125,
             a_of=lambda z: 0, b_of=lambda z: z * GD)


def test_zz_tally(env):
    """Every family ran; the tally is printed (and written to PTK_GEMM_CONTRACT_REPORT)."""
    if not TALLY:      # (run on its own: nothing to report)
        return
    print(json.dumps(TALLY, indent=1, sort_keys=True))
    path = os.environ.get("PTK_GEMM_CONTRACT_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(TALLY, f, indent=1, sort_keys=True)
    for t in TALLY.values():
        assert all(v <= G.NEQ_CAP for v in t["neq"].values()), t
