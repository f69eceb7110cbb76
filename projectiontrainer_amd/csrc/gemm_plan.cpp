// The GEMM dispatch planner: which kernel family, tile height, stream-K tail and K split a GEMM shape gets.
// Every shape rule of launch_gemm (gemm.hip), gemm_split (models.cpp) and the persistent kernels' launchers
// (gemm_w4.hip, gemm_tn.hip) lives here as a pure host function of the operands and a GemmPlanEnv (the CU count, the
// test force mode, the A/B switches, the lent tail scratch): no kernels, no HIP calls, no environment reads, no
// globals, so ptk_gemm_plan / ptk_gemm_split_plan answer "what does shape X dispatch to" without a GPU
// (tests/test_gemm_plan.py).  The measurement comments say why each threshold stands where it does.
#include <algorithm>

#include "ptk_internal.h"

namespace ptk {

// ============================================================================ what the persistent kernels take
// the W4 path needs: batch 1, 16-B aligned rows of every operand it touches 8 columns at a time,
// N % 8 == 0, byte extents of A and B below 2^31 (32-bit buffer offsets)
bool w4_supported(const GemmArgs& a, int act, int out) {
  if (a.N % 8 || a.K % W4_KT) return false;
  if (a.alpha != 1.f) return false;   // the persistent epilogues take the accumulators as they are (no scale)
  if (a.row_stats) return false;   // the softmax-statistics epilogue lives in gemm.hip's epilogue only
  if (a.resid16 && (out != OUT_BF16 || a.ld_resid16 % 8)) return false;
  if ((a.ldc % 8) || (a.resid && a.ld_resid % 4) || (a.rowadd && a.ld_rowadd % 4)) return false;
  if ((a.aux || a.aux2) && a.ld_aux % 8) return false;
  if ((a.aux_in || a.aux_in2) && a.ld_aux_in % 8) return false;
  if (((uintptr_t)a.C | (uintptr_t)a.bias | (uintptr_t)a.resid | (uintptr_t)a.resid16 | (uintptr_t)a.rowadd | (uintptr_t)a.aux |
       (uintptr_t)a.aux2 | (uintptr_t)a.aux_in | (uintptr_t)a.aux_in2) & 15)
    return false;
  if (act == ACT_GEGLU && (a.N % 32)) return false;
  if (act == ACT_GEGLU_BWD && (!a.aux_in || !a.aux_in2 || (a.N % 16) || (a.ldc % 8))) return false;
  if (act == ACT_GELU_ERF_BWD && !a.aux_in) return false;
  if (out != OUT_BF16 && (act != ACT_NONE)) return false;
  if (a.amap.g != 0) return false;   // gathered A rows: not an affine row panel
  const double abytes = (double)(a.M + a.amap.off) * a.lda * 2, bbytes = (double)a.N * a.ldb * 2;
  return abytes < 2147483000.0 && bbytes < 2147483000.0;
}

// the p8 path takes what the w4 path takes, at K >= 128 (a tile's first and last k-step pairs are peeled)
bool p8_supported(const GemmArgs& a, int act, int out) { return a.K >= 128 && w4_supported(a, act, out); }

double w4_round_fill(long M, long N, int ncu) {
  const long ntile = ((M + W4 - 1) / W4) * ((N + W4 - 1) / W4), cu = ncu;
  return (double)ntile / (double)(((ntile + cu - 1) / cu) * cu);
}

// the lean bf16 epilogue (gemm_persist.h w4_epilogue_lean) applies: ACT_NONE / ACT_GELU_TANH into bf16 with at most
// a bias, the bf16-linear rounding and a bf16 residual (row-aligned with C, 16-B rows); a C row map that is an
// offset (cmap.g == 0, or a group map without skipped rows whose group stride equals its size: the identity
// plus cmap.off); whole 64-column wave ranges (the 4-wave kernel, whose waves hold 128 columns, asks for N % 128
// itself: launch_gemm_w4); C's extent (rows cmap.off .. M + cmap.off) below 2^31 bytes.
// c_bytes = that extent (num_records of the store resource: rows past M are dropped).  lean_epi false
// (PTK_LEAN_EPI=0 in A/B builds, PTK_AB) keeps the general epilogue (bit-identical either way)
// the lean GEGLU-backward epilogue (w4_epilogue_lean_glu): the saved g, u inputs with 16-B rows, no other epilogue
// input, an offset C row map, whole 128-column wave ranges, extents below 2^31 bytes
// (kt: its k-step-tiled form, which skips a wave's column pairs past N one by one: whole k-steps of N suffice)
static bool lean_glu_ok(const GemmArgs& a, int act, int out, uint32_t& c_bytes, bool lean_epi, bool kt = false) {
  if (!lean_epi || act != ACT_GEGLU_BWD || out != OUT_BF16) return false;
  if (a.bias || a.rowadd || a.resid || a.resid16 || a.bf16_linear || a.row_stats || a.alpha != 1.f) return false;
  const bool affine = a.cmap.g == 0 || (a.cmap.skip == 0 && a.cmap.gs == a.cmap.g);
  if (!affine || a.cmap.off < 0 || a.amap.g != 0 || a.N % (kt ? 32 : 128) || a.ldc % 8 || ((uintptr_t)a.C & 15))
    return false;
  if (!a.aux_in || !a.aux_in2 || a.ld_aux_in % 8 || a.ld_aux_in < a.N) return false;
  if (((uintptr_t)a.aux_in | (uintptr_t)a.aux_in2) & 15) return false;
  if (a.ldc < 2 * a.N) return false;
  const double side = (double)a.M * (double)a.ld_aux_in * 2.0;
  const double bytes = ((double)a.M + (double)a.cmap.off) * (double)a.ldc * 2.0;
  if (bytes >= 2147483000.0 || side >= 2147483000.0) return false;
  c_bytes = (uint32_t)bytes;
  return true;
}
bool lean_epilogue_ok(const GemmArgs& a, int act, int out, uint32_t& c_bytes, bool lean_epi) {
  if (act == ACT_GEGLU_BWD) return lean_glu_ok(a, act, out, c_bytes, lean_epi, a.c_kt != 0);
  if (!lean_epi || (act != ACT_NONE && act != ACT_GELU_TANH) || out != OUT_BF16) return false;
  if (a.rowadd || a.resid || a.aux || a.aux2 || a.aux_in || a.aux_in2 || a.row_stats || a.alpha != 1.f) return false;
  const bool affine = a.cmap.g == 0 || (a.cmap.skip == 0 && a.cmap.gs == a.cmap.g);
  if (!affine || a.cmap.off < 0 || a.N % 64 || a.ldc % 8 || a.ldc < a.N || ((uintptr_t)a.C & 15)) return false;
  if (a.bias && ((uintptr_t)a.bias & 15)) return false;
  if (a.resid16 && (a.ld_resid16 % 8 || ((uintptr_t)a.resid16 & 15))) return false;
  const double rows = (double)a.M + (double)a.cmap.off;
  const double bytes = rows * (double)a.ldc * 2.0, rbytes = a.resid16 ? rows * (double)a.ld_resid16 * 2.0 : 0.0;
  if (bytes >= 2147483000.0 || rbytes >= 2147483000.0) return false;
  c_bytes = (uint32_t)bytes;
  return true;
}

bool lean_epilogue_candidate(const GemmArgs& a, bool lean_epi) {
  uint32_t cb = 0;
  return lean_epilogue_ok(a, ACT_NONE, OUT_BF16, cb, lean_epi);
}

// ============================================================================ the stream-K tail
size_t p8_slab_bytes(long G) { return (size_t)G * 2 * 8 * P8_WAVE_FLOATS * sizeof(float); }

// the stream-K plan of a launch.  Cost model of the tail round, in K-tiles of one workgroup (a 256x256x64 step,
// ~1.3 us): unsplit, nt; split over Gs workgroups, ceil(U / Gs) plus the partial writes of a workgroup's (at most
// two) cut pieces (a 256-KiB slab each, ~1 K-tile) and the fixup launch (~5 K-tiles).  The cheapest Gs is taken
// when it saves >= 10 % of the round.
P8Tail p8_tail_plan_ws(const GemmArgs& a, long ntile, long G, void* slab, long max_t0, long max_t1) {
  P8Tail tl;
  const long R = ntile / G, T = ntile - R * G, nt = a.K / W4_KT;
  if (!slab || T == 0 || (nt & 1)) return tl;
  if (!((R == 0 && T <= max_t0) || (R == 1 && T <= max_t1))) return tl;
  const long U = T * (nt / 2);                                // tail units: pairs of K-tiles
  double best = (double)nt * 0.9;
  long bestG = 0;
  for (long gs = T + 1; gs <= G; ++gs) {
    const long per = (U + gs - 1) / gs;                       // units of the busiest workgroup
    if (U / gs < 1) break;                                    // (every workgroup >= 1 unit)
    const double cost = 2.0 * (double)per + 2.0 + 5.0;
    if (cost < best - 1e-9) { best = cost; bestG = gs; }
  }
  if (!bestG || R + 3 > 64 || G > 1023 || ntile > 65535) return tl;   // the kernel's per-lane segment table
  tl.dp_tiles = (int)(R * G);
  tl.units = (int)U;
  tl.gsplit = (int)bestG;
  tl.slab = (float*)slab;
  return tl;
}

// the 8-wave kernel's plan: the scratch of the descriptor or the model-level scope (slabs after the counters).
// Long K only (K >= 4096: the fixup launch and the partial writes cost a few K-tiles), and a tail the split
// shortens without losing the lock-step L2 sharing of a round: a grid of at most 64 tiles, or one full round plus
// at most 128.  Measured (tools/sk_ab.py, r05, same box): SigLIP fc2 0.90x, projector fc2 0.91x, Stage 2's
// down / d(gate|up) dX 0.72 / 0.63x, projector dW1 (160 tiles, no full round) 0.90x; slower where many tiles
// share no full round (projector dW2 200 tiles 1.31x, the Stage-2 SigLIP fc2 144 tiles 1.11x, Gemma's 440-tile
// projections with 184 tail tiles 1.06-1.08x)
P8Tail p8_tail_plan(const GemmArgs& a, int act, int out, const GemmPlanEnv& env) {
  void* ws = a.tail_ws ? a.tail_ws : env.tail_scope;
  if (!ws || act != ACT_NONE || (out != OUT_BF16 && out != OUT_F32 && out != OUT_F32_BFR)) return P8Tail{};
  if (a.K < 4096) return P8Tail{};
#ifndef PTK_SK_MAXT1
#define PTK_SK_MAXT1 128   // A/B builds (make ablib AB_SRC=gemm_plan.cpp AB_DEFS=-DPTK_SK_MAXT1=..) vary the one-round-plus-tail limit
#endif
  const long ntile = (long)((a.M + W4 - 1) / W4) * ((a.N + W4 - 1) / W4);
  return p8_tail_plan_ws(a, ntile, env.ncu, (char*)ws + P8_CNT_BYTES, 64, PTK_SK_MAXT1);
}

// ============================================================================ the tile height of the 8-wave kernel
// the tile height of a plain / GELU-tanh 8-wave GEMM without a stream-K tail: the TM of {256, 224, 192, 160} with the
// lowest tile rounds x (TM + 128), a tie with 256 rows going to the shorter tile (SigLIP fc1: 6 rounds of 192 = 5 of
// 256; +0.15 % on the cfg2 step over three same-box alternations, profiles/r05_tm160_ab.txt; with a 5 % margin it
// stayed at 256).  The 128 rows' worth per round is what shorter tiles do not shed (prologue, epilogue, the DMA / LDS work per MFMA): fitted to tools/p8_probe.py
// (r05, same box): Gemma o 59.6 / 54.1 / 68.5 us at 256 / 224 / 192 rows, dO 65.8 / 59.5 / 54.4, q|k|v 90.7 / 88.0
// / 81.4, down 340 / 312 / 407, SigLIP fc1 149 / 157 / 153 (on another box 154.7 at 256, 148.1 at 192); 160 rows:
// SigLIP o 52.1 -> 46.4 us (2 rounds of 160 vs 2 of 192), Gemma dO stays at 192 (57.6 vs 70.9), profiles/r05_tm160_ab.txt
int p8_tile_height(const GemmArgs& a, int act, int out, int ncu) {
  if (!(act == ACT_NONE || (act == ACT_GELU_TANH && out == OUT_BF16))) return 256;
  const long nbn = (a.N + W4 - 1) / W4, cu = ncu;
  auto cost = [&](long tm) { return (double)((((a.M + tm - 1) / tm) * nbn + cu - 1) / cu) * (double)(tm + 128); };
  const double c256 = cost(256);
  int best = 256;
  double bc = c256;
  for (int tm : {224, 192, 160}) {
    const double c = cost(tm);
    if (c < bc || (c == bc && best == 256)) { bc = c; best = tm; }   // a tie with 256 rows goes to the shorter tile
  }
  return best;
}

// ============================================================================ launch_gemm's rule
// One ordered list of named predicates; gemm_plan below reads them in launch order.
namespace {

bool plain_bf16_or_f32(int act, int out) { return act == ACT_NONE && (out == OUT_BF16 || out == OUT_F32); }
long tiles256(const GemmArgs& a) { return (long)((a.M + 255) / 256) * ((a.N + 255) / 256); }
// where the shape rule (not a force mode) may pick a persistent kernel
bool persistent_range(const GemmArgs& a, const GemmPlanEnv& e) {
  return e.force_tiles == 0 && a.M >= 4096 && a.N <= 16384;
}

// single-round.  r05: a plain bf16 grid of one partial round of 256x256 tiles beats the 128x128 kernel's
// ~1.1 rounds of two blocks per CU (tools/sk_ab.py, Stage 2's SigLIP at M = 9 216: o 31.3 vs
// 41.8 us, fc2 85.1 vs 109.1; its down projection at bs 8 133.6 vs 177.8).  gemm_split_plan keeps such a shape
// unsplit: the 8-wave kernel unsplit beats the split-K 128x128 slices (Stage 2 at bs 8: the down projection 133.6
// vs 177.8 us); K <= 8192, so a longer K (Gemma3-4B's down projection, K 10 240) keeps the split
bool single_round(const GemmArgs& a, int act, int out, const GemmPlanEnv& e) {
  return persistent_range(a, e) && act == ACT_NONE && out == OUT_BF16 && a.K <= 8192 && tiles256(a) <= e.ncu &&
         lean_epilogue_candidate(a, e.lean_epi);
}

// short-tile.  224- / 192-row tiles on the 8-wave kernel where their rounds undercut the 256-row ones (p8_tile_height:
// Gemma3's N 1152 / 1536 / 1024 projections at M 22 528, SigLIP's q|k|v, o and fc1 at M 18 432), ahead of the
// 4-wave and 128x128 kernels; force modes 512 / 1024 / 4096 put every plain / GELU-tanh single GEMM on 224 / 192 /
// 160 rows (tests).  tm_short false (PTK_TM224=0 in A/B builds, PTK_AB): 256-row tiles only.  Only without a
// stream-K tail (the tail kernel has 256-row tiles)
int short_tile(const GemmArgs& a, int act, int out, const GemmPlanEnv& e) {
  if (!(act == ACT_NONE || (act == ACT_GELU_TANH && out == OUT_BF16))) return 256;
  if (e.force_tiles == 0 && e.tm_short && a.M >= 4096) return p8_tile_height(a, act, out, e.ncu);
  if (e.force_tiles == 512) return 224;
  if (e.force_tiles == 1024) return 192;
  if (e.force_tiles == 4096) return 160;
  return 256;
}

// tail.  The stream-K tail (gemm_w4.hip P8Tail): a plain GEMM whose last tile round fills the CUs badly, with tail
// scratch lent by the model-level call (or in the descriptor), runs on the persistent 8-wave kernel with that
// round's K-tiles spread over the CUs (r04: the N = 1024 / 1152 / 1536 projections, the long-K d(gate|up) dX
// and down projection, the projector's fc2 and weight grads)
P8Tail tail(const GemmArgs& a, int act, int out, const GemmPlanEnv& e) {
  if (!((e.force_tiles == 0 || e.force_tiles == 32) && act == ACT_NONE && a.M >= 1024 && a.N >= 256 && a.N <= 16384))
    return P8Tail{};
  return p8_tail_plan(a, act, out, e);
}

// w4.  Persistent 4-wave 256x256 kernel (gemm_w4.hip) where it measured ahead of the 8-wave and
// 128x128 kernels (tools/gemm_bench.py --all, same box, r01): the GEGLU gate|up projection, and
// plain projections (bf16 or fp32 out, K <= 8192) whose 256x256 tiles fill >= 80 % of the
// persistent grid's rounds (SigLIP qkv +4 %, Gemma o +6 %, dh +17 %, down +3 %, dqkv +2 %).  Not the
// N = 1024 / 1536 shapes (352 / 528 tiles: 69 % round fill, the 128x128 kernel wins), the
// vocab-wide lm_head, the K = 11520 / 13824 projections or the GELU epilogues
// (r02: + the GELU-tanh epilogue with packed f32 math, SigLIP fc1 887 -> 936 TFLOP/s, tools/gemm_bench.py --all)
bool w4_shape(const GemmArgs& a, int act, int out, const GemmPlanEnv& e) {
  return persistent_range(a, e) &&
         (act == ACT_GEGLU || act == ACT_GEGLU_BWD ||
          ((plain_bf16_or_f32(act, out) || (act == ACT_GELU_TANH && out == OUT_BF16)) && a.K <= 8192 &&
           w4_round_fill(a.M, a.N, e.ncu) >= 0.8));
}

// p8-over-w4.  Persistent 8-wave kernel (two waves per SIMD, gemm_w4.hip) where it measured ahead of the 4-wave one
// (tools/p8_probe.py, same box, interleaved, r03): the w4 plain / GELU-tanh shapes at K <= 2048 (Gemma q|k|v
// 90 -> 87 us, o 58 -> 56, SigLIP q|k|v 111 -> 109, fc1 157 -> 151), the projector fc1 with the GELU-erf
// epilogue (674 -> 583 us) and its backward (dA, 858 -> 703 us) and the long-K d(gate|up) dX (K 13 824, N <= 2048: 700 -> 672 us); w4 keeps the
// GEGLU / GEGLU-backward epilogues and the K 6 912 down projection (697 / 486 / 330 us vs 723 / 500 / 342).
// p8_all (PTK_P8=1 in A/B builds, PTK_AB) puts every w4 shape on it
// (the two-group persistent kernel on 256x128 tiles, gemm_dual.hip, measured 17-44 % slower than the 8-wave
// kernel in round 5, profiles/r05_dual_probe.txt, and was removed from the tree in round 6)
bool p8_over_w4(const GemmArgs& a, int act, int out, const GemmPlanEnv& e) {
  if (!persistent_range(a, e)) return false;
  const double fill = w4_round_fill(a.M, a.N, e.ncu);
  return (w4_shape(a, act, out, e) && (e.p8_all || (act != ACT_GEGLU && act != ACT_GEGLU_BWD && a.K <= 2048))) ||
         ((act == ACT_GELU_ERF || act == ACT_GELU_ERF_BWD) && out == OUT_BF16 && a.K <= 2048 && fill >= 0.8) ||
         (plain_bf16_or_f32(act, out) && a.K >= 12288 && a.N <= 2048) ||
         // r05: with the lean bf16 epilogue the 8-wave kernel also beats the 128x128 one on the N 1536
         // projection at 69 % round fill (Gemma q|k|v 90.7 vs 95.3 us, profiles/r05_dual_solo_probe.txt);
         // the N 1024 ones stay on 128x128 (dO 66.0 vs 63.2, SigLIP fc2 187 vs 171)
         (act == ACT_NONE && out == OUT_BF16 && a.N >= 1536 && a.K <= 2048 && fill >= 0.65 &&
          lean_epilogue_candidate(a, e.lean_epi));
}

// big / staggered-big.  256x256 (one block per CU) only where the K loop amortises its lock-step epilogue: long K or
// wide N at K >= 1152.  Elsewhere two co-resident 128x128 blocks per CU overlap one block's
// epilogue with the other's MFMA and quantise better (tools/gemm_bench.py --all, r01).
bool big_shape(const GemmArgs& a) {
  return a.M >= 1024 && a.N >= 512 && (a.K >= 6144 || (a.N >= 6144 && a.K >= 1152));
}
// long K: the barrier-staggered 256x256 variant (+6-7 % at K >= 4096, tools/gemm_bench.py --all)
bool staggered_big(const GemmArgs& a, const GemmPlanEnv& e) {
  return e.force_tiles == 4 || (e.force_tiles == 0 && big_shape(a) && a.K >= 4096);
}
bool big(const GemmArgs& a, const GemmPlanEnv& e) {
  return e.force_tiles != 1 && (e.force_tiles == 2 || big_shape(a));
}

}  // namespace

// Force modes (tests): 1 = every GEMM on 128x128, 2 / 4 = single-batch GEMMs on 256x256 / staggered 256x256, 8 / 32 =
// the persistent 4-wave / 8-wave kernel wherever they are supported, 512 / 1024 / 4096 = short tiles (short_tile).
// Batched GEMMs (split-K slices, attention-shaped batches) always run on the 128x128 kernel.
GemmPlan gemm_plan(const GemmArgs& a, int act, int out, int batch, const GemmPlanEnv& e) {
  GemmPlan p;
  if (batch != 1) {
    p.path = GEMM_PATH_NTB;
    return p;
  }
  if (p8_supported(a, act, out)) {
    const P8Tail tl = tail(a, act, out, e);
    const int tm = tl.units ? 256 : short_tile(a, act, out, e);
    const bool single = single_round(a, act, out, e);
    if (e.force_tiles == 32 || single || tl.units || tm != 256 || p8_over_w4(a, act, out, e)) {
      p.path = tl.units ? GEMM_PATH_P8SK : GEMM_PATH_P8;
      p.tm = tm;
      p.tail = tl;
      p.single_round = single;
      return p;
    }
  }
  if ((e.force_tiles == 8 || w4_shape(a, act, out, e)) && w4_supported(a, act, out)) p.path = GEMM_PATH_W4;
  else if (staggered_big(a, e)) p.path = GEMM_PATH_BIG2;
  else if (big(a, e)) p.path = GEMM_PATH_BIG;
  return p;
}

// ============================================================================ the k-step-tiled copy of B
// The persistent kernels stage B in 1-KiB pieces: 16 rows x one 32-deep k-step, lane i fetching row i >> 2, logical
// 16-B chunk (i & 3) ^ ((i >> 3) & 2) (gemm_w4.hip).  From row-major B that is 16 half lines per piece; the tiled
// copy stores each piece as the contiguous KiB its lanes write to LDS, 8 whole 128-B lines, the k-steps of a 16-row
// group g one after the other: block (g, s) at byte (g K/32 + s) 1024, unit i of it as above.  So element (row, k)
// sits in unit 4 (row & 15) + (chunk ^ ((row >> 1) & 2)) of block (row / 16, k / 32), chunk = (k / 8) & 3.  Groups
// are ordered row-major: every row >= N lies at or past byte N K 2, outside the buffer range, and reads as zero.
long kstep_tile_offset(long row, long k, long K) {
  const long rr = row & 15, chunk = (k >> 3) & 3;
  const long unit = 4 * rr + (chunk ^ ((rr >> 1) & 2));
  return ((row >> 4) * (K / 32) + (k >> 5)) * 1024 + unit * 16 + (k & 7) * 2;
}

// a launch reads B_kt only on the families whose B pieces are 16 rows x 64 B, at batch 1, from a packed B (ldb ==
// K), under an epilogue that has a tiled kernel variant (bkt_act).  K slices never take it either (a slice's k-steps
// are not a prefix of a group's stream), but no plan that reaches launch_gemm carries slices: their callers drop the
// pointer themselves (gemm_split in models.cpp, launch_gemm_p8_kslices in gemm_w4.hip)
bool b_ktiled_ok(const GemmArgs& a, const GemmPlan& plan, int act, int batch) {
  if (!a.B_kt || batch != 1 || !bkt_act(act)) return false;
  if (plan.path != GEMM_PATH_W4 && plan.path != GEMM_PATH_P8 && plan.path != GEMM_PATH_P8SK) return false;
  return a.ldb == a.K && a.K % 32 == 0 && a.N % 16 == 0 && !((uintptr_t)a.B_kt & 15);
}

// The activation form: the same layout over A [M][K].  Only the 8-wave kernel has the variant (gemm_w4.hip AKT), on
// whole tiles (no stream-K tail: a cut tail's kernel has none) with a plain bf16 epilogue and a tiled B.  A
// tile's first 16-row group must start where its first row does: M % 16 == 0 makes every group wholly valid or
// wholly past the buffer's end (reads zero), every tile height is a multiple of 16, and the row offset must be one
bool a_ktiled_ok(const GemmArgs& a, const GemmPlan& plan, int act, int out, int batch, bool lean_epi) {
  if (batch != 1 || act != ACT_NONE || out != OUT_BF16 || plan.path != GEMM_PATH_P8 || plan.tail.units) return false;
  if (a.M % 16 || a.K % 32 || a.lda != a.K || a.amap.g != 0 || a.amap.off < 0 || a.amap.off % 16) return false;
  (void)lean_epi;   // (the lean and the general plain bf16 epilogues both have the variant)
  return b_ktiled_ok(a, plan, act, batch);
}

// The producers: the 4-wave kernel's GEGLU epilogue (h [M][N / 2], with aux_kt the factors a, b beside it) and its
// lean GEGLU-backward epilogue (dg | du [M][2 N], with aux_in_kt the factors read tiled), each with a tiled B.  A
// tiled width of whole k-steps, packed outputs, an identity C row map with a 16-aligned offset
bool c_ktiled_ok(const GemmArgs& a, const GemmPlan& plan, int act, int out, int batch, bool lean_epi) {
  if (!a.c_kt) return !a.aux_kt && !a.aux_in_kt;   // (the factors go tiled only beside a tiled output)
  if (batch != 1 || out != OUT_BF16 || plan.path != GEMM_PATH_W4 || a.M % 16 || !b_ktiled_ok(a, plan, act, batch))
    return false;
  if (a.cmap.g != 0 || a.cmap.off < 0 || a.cmap.off % 16 || ((uintptr_t)a.C & 15)) return false;
  if (act == ACT_GEGLU) {
    if (a.N % 64 || a.ldc != a.N / 2 || a.aux_in_kt) return false;
    return !a.aux_kt || (a.aux && a.aux2 && a.ld_aux == a.N / 2 && !(((uintptr_t)a.aux | (uintptr_t)a.aux2) & 15));
  }
  uint32_t cb = 0;
  if (act != ACT_GEGLU_BWD || a.aux_kt || !lean_epilogue_ok(a, act, out, cb, lean_epi)) return false;
  return a.ldc == 2L * a.N && (!a.aux_in_kt || a.ld_aux_in == a.N);
}

// One decision per producer / consumer pair, made before the producer is launched (the consumer is planned later, and
// through gemm_split): the producer writes its output tiled (and the GEGLU factors with `factors`) and the consumer
// reads it as a tiled A only if the producer's plan is the 4-wave kernel with that epilogue, gemm_split_plan leaves
// the consumer unsplit and without a lent tail, the consumer's plan (the split plan's direct one; under a force mode
// the launch plans again, so that plan) has the tiled-A variant, and both sets of operands qualify.  prod / cons:
// the operands as they will be launched, flags unset.  enabled: the run-time switch (PTK_A_KTILED)
bool gemm_ktiled_pair(const GemmArgs& prod, int pact, const GemmArgs& cons, long part_floats, const GemmPlanEnv& env,
                      bool enabled, bool factors) {
  if (!enabled || (pact != ACT_GEGLU && pact != ACT_GEGLU_BWD)) return false;
  GemmArgs p = prod, c = cons;
  p.c_kt = 1;
  if (factors) (pact == ACT_GEGLU ? p.aux_kt : p.aux_in_kt) = 1;
  c.a_kt = 1;
  if (!c_ktiled_ok(p, gemm_plan(prod, pact, OUT_BF16, 1, env), pact, OUT_BF16, 1, env.lean_epi)) return false;
  if (cons.A != (const bf16_t*)prod.C || cons.M != prod.M || cons.K != (pact == ACT_GEGLU ? prod.N / 2 : 2 * prod.N) ||
      cons.amap.off != prod.cmap.off)
    return false;
  const GemmSplitPlan sp = gemm_split_plan(cons, OUT_BF16, part_floats, env);
  if (sp.kc != 0 || sp.tail_ws) return false;
  const GemmPlan cp = env.force_tiles == 0 ? sp.direct : gemm_plan(cons, ACT_NONE, OUT_BF16, 1, env);
  return a_ktiled_ok(c, cp, ACT_NONE, OUT_BF16, 1, env.lean_epi);
}

// ============================================================================ gemm_split's rule
// Split-K for long-K GEMMs whose 256x256 tile grid fills few of the CUs' rounds (measured, tools/splitk_probe.py
// r02: the cfg4 shapes dW_qkv 313 -> 73 us and dW_o 313 -> 68 us at 4 slices; dW_down, dW_gate|up, the
// d(gate|up) dX and the down projection at 280 tiles -8..-16 % at 2 slices; the cfg2 d(gate|up) dX at 440
// tiles is slower split, the vocab-wide lm_head dW too).  part_floats: the fp32 scratch for the partials (0: none).
// The decision is the default dispatch's: a test force mode acts at each launch, not on the split.
GemmSplitPlan gemm_split_plan(const GemmArgs& a, int out, long part_floats, const GemmPlanEnv& env) {
  GemmSplitPlan sp;
  GemmPlanEnv e = env;
  e.force_tiles = 0;
  // the persistent kernel's stream-K tail takes the shapes it measured faster on (p8_tail_plan: Stage 2's weight
  // grads and M = 14 336 projections) before any host-side split; so does the single-round rule
  sp.direct = gemm_plan(a, ACT_NONE, out, 1, e);
  const GemmPlan& direct = sp.direct;
  if (direct.path == GEMM_PATH_P8SK) return sp;
  // long-K GEMMs whose 256x256 tiles leave a thin last round (Stage 2's d(gate|up) dX and down projection at M =
  // 14 336: 280 tiles = 256 + 24): the 8-wave kernel's stream-K tail over the split-K scratch, its pieces summed by
  // p8_fixup_kernel (r05, tools/sk_ab.py same box: 419 / 216 us vs 662 / 298 unsplit; the 2-slice 128x128 split
  // below ran them at ~390 + 26 us on average)
  if (e.streamk && a.K >= 4096 && (size_t)part_floats * sizeof(float) >= P8_CNT_BYTES + p8_slab_bytes(e.ncu)) {
    GemmArgs b = a;
    b.tail_ws = reinterpret_cast<void*>((uintptr_t)256);   // (any scratch: the caller points the plan's slab at the real one)
    const GemmPlan lent = gemm_plan(b, ACT_NONE, out, 1, e);
    if (lent.path == GEMM_PATH_P8SK) {
      sp.tail_ws = true;
      sp.direct = lent;
      return sp;
    }
  }
  if (direct.single_round) return sp;
  const long nbig = tiles256(a);
  int S = 1, kmin = 1024;
  if (a.K >= 4096 && nbig <= 64) S = 4;
  else if (a.K >= 4096 && nbig <= 300) S = 2;
  // small M (cfg1, bs 2: M = 520): the 128x128 tile grid alone leaves most CUs idle, so split K until
  // the slices fill about two blocks per CU (slices >= 256 deep)
  const long n128 = (long)((a.M + 127) / 128) * ((a.N + 127) / 128), cus = e.ncu;
  if (n128 * 2 <= cus) {
    kmin = 256;
    while (n128 * S * 2 <= 2 * cus && a.K / (S * 2) >= kmin) S *= 2;
  }
  while (S > 1 && ((long)S * a.M * a.N > part_floats || a.K / S < kmin || a.N % 4 || a.ldc % 4)) S /= 2;
  const bool plain = !a.rowadd && !a.resid && !a.aux && !a.aux_in && a.amap.g == 0 && a.amap.off == 0 &&
                     a.cmap.g == 0 && a.cmap.off == 0 && a.bias == nullptr && a.alpha == 1.f;
  if (S == 1 || !plain) return sp;
  sp.kc = (a.K / S + 63) / 64 * 64;
  sp.slices = a.K / sp.kc;
  sp.rem = a.K - sp.slices * sp.kc;
  return sp;
}

// ============================================================================ the token-major weight-grad GEMM
// the TN path takes: 16-B aligned operands with 16-B k-rows, K split into `slices` equal slices of >= 128 rows (a
// multiple of 64), N % 64 == 0, operand extents below 4 GiB and C's below 2^31; OUT_BF16 only with the lean epilogue's form (the weight-grad
// accumulate: bf16_linear + resid16), OUT_F32 the partials of a K split ([slices][M][ldc])
bool tn_supported(const GemmArgs& a, int out, int slices, bool lean_epi) {
  if (slices < 1 || a.K % (W4_KT * slices) || a.K / slices < 2 * W4_KT) return false;
  if (a.N % 64 || a.lda % 8 || a.ldb % 8 || a.lda < a.M || a.ldb < a.N) return false;
  if (((uintptr_t)a.A | (uintptr_t)a.B | (uintptr_t)a.C) & 15) return false;
  if (a.amap.g || a.amap.off || a.bias || a.rowadd || a.resid || a.aux || a.aux_in || a.row_stats || a.alpha != 1.f)
    return false;
  // operand extents below 4 GiB less 1 MiB: 32-bit buffer offsets and num_records (the tied lm_head's dW reads the
  // 2 GiB d(logits) [4 096][262 144]); the last tile's read past its k-row never wraps
  const double ab = (double)a.K * a.lda * 2, bb = (double)a.K * a.ldb * 2;
  if (ab >= 4293918720.0 || bb >= 4293918720.0) return false;
  if (out == OUT_BF16) {
    uint32_t cb = 0;
    return slices == 1 && lean_epilogue_candidate(a, lean_epi) && lean_epilogue_ok(a, ACT_NONE, OUT_BF16, cb, lean_epi);
  }
  if (out != OUT_F32 || a.ldc % 4 || a.ldc < a.N || a.cmap.g || a.cmap.off || a.resid16 || a.bf16_linear) return false;
  return (double)slices * a.M * a.ldc * 4 < 2147483000.0;
}

// Slice count of a weight grad (a: the OUT_BF16 accumulate form).  Cost in us: the tile rounds of the persistent
// grid, each K / S / 64 K-tiles of ~1.15 us (a 256x256x64 step at ~75 % of one CU's MFMA rate) plus ~4 us of
// epilogue, and for S > 1 the fp32 partials written, read back and reduced with the bf16 accumulate
// ((8 S + 4) M N bytes at ~5 TB/s).  cfg4: dW_gate|up (54 x 5 tiles, K 14 336) 2 slices (partials capped by the
// workspace), dW_down (5 x 27) 1, dW_qkv (6 x 5) and dW_o (5 x 4) 8
int tn_slices(const GemmArgs& a, long part_floats, const GemmPlanEnv& env) {
  const long tiles = (long)((a.M + W4 - 1) / W4) * ((a.N + W4 - 1) / W4), cu = env.ncu;
  int best = 0;
  double best_us = 0;
  for (int S = 1; S <= 16; S *= 2) {
    GemmArgs f = a;
    int out = OUT_BF16;
    if (S > 1) {
      if ((double)S * a.M * a.N > (double)part_floats) break;
      f.C = reinterpret_cast<void*>((uintptr_t)256);   // (the partials' alignment is the workspace's, checked at launch)
      f.ldc = a.N;
      f.bf16_linear = 0;
      f.resid16 = nullptr;
      f.ld_resid16 = 0;
      out = OUT_F32;
    }
    if (!tn_supported(f, out, S, env.lean_epi)) continue;
    const long rounds = (tiles * S + cu - 1) / cu;
    const double us = (double)rounds * ((double)a.K / S / W4_KT * 1.15 + 4.0) +
                      (S > 1 ? (8.0 * S + 4.0) * (double)a.M * a.N / 5e6 : 0.0);
    if (!best || us < best_us) { best = S; best_us = us; }
  }
  return best;
}

// the stream-K plan of a one-slice TN GEMM over `slab` (p8_slab_bytes(CUs) bytes): any tail of at most 256 tiles
// without a full round before it (the few-tile weight grads: dW_down 135 tiles, dW_qkv 30, dW_o 20), at most 64
// after one (dW_gate|up: 270 = 256 + 14)
P8Tail tn_tail_plan(const GemmArgs& a, void* slab, int ncu) {
  const long ntile = (long)((a.M + W4 - 1) / W4) * ((a.N + W4 - 1) / W4);
  return p8_tail_plan_ws(a, ntile, ncu, slab, 256, 64);
}

}  // namespace ptk
