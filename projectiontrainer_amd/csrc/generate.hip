// Kernels of the KV-cache decode (ptk_gemma3_generate, models.cpp): the validation `generate` of the Stage-1
// trainer (Stage1/projector_trainer.py:386-393: unwrapped_llm.generate(inputs_embeds=projected_embeds,
// attention_mask=ones, max_new_tokens=64, do_sample=True, pad_token_id, eos_token_id)) and of Stage 2
// (Stage2/trainer.py:626).  The layers themselves run on the training path's kernels; what is new here is
//   * the prompt copy into the padded prefill layout (+ its key-valid mask),
//   * the K / V cache append (the prefill's rows, then one row per decode step),
//   * the per-row sampling step: HF generate's logits processors for do_sample (temperature, then top-k: every
//     logit below the k-th largest dropped, ties kept -- TF/generation/logits_process.py TopKLogitsWarper), a
//     softmax draw over what is left, or greedy argmax (first index of the maximum, as torch.argmax), and the
//     finished-sequence rule of GenerationMixin._sample (a row that produced eos_token_id emits pad_token_id).
#include "common.h"
#include "ptk_internal.h"

namespace ptk {

// prompt rows b*ld_b + i (i < P, fp32 [.., H]) -> x rows b*Pp + i; rows P..Pp-1 zero; key_valid = (i < P)
__global__ void __launch_bounds__(256) gen_prompt_kernel(const float* __restrict__ src, long ld_b, int P, int Pp,
                                                         int H, float* __restrict__ x, int32_t* __restrict__ kv) {
  const long row = blockIdx.x;
  const int b = (int)(row / Pp), i = (int)(row - (long)b * Pp);
  if (threadIdx.x == 0) kv[row] = i < P;
  float* xr = x + row * H;
  const float* sr = src + ((long)b * ld_b + i) * H;
  for (int c = threadIdx.x * 4; c < H; c += 1024)
    *reinterpret_cast<float4*>(xr + c) = i < P ? *reinterpret_cast<const float4*>(sr + c) : make_float4(0, 0, 0, 0);
}
int launch_gen_prompt(const float* src, long ld_b, int B, int P, int Pp, int H, float* x, int32_t* kv,
                      hipStream_t st) {
  if (H % 4 || P > Pp) return set_error("generate: prompt layout (H %% 4, P <= Pp)");
  hipLaunchKernelGGL(gen_prompt_kernel, dim3((unsigned)((long)B * Pp)), dim3(256), 0, st, src, ld_b, P, Pp, H, x, kv);
  return hipGetLastError() == hipSuccess ? 0 : set_error("gen_prompt launch failed");
}

// rows [0, n) of each z of src [Z][src_z / D][D] -> rows p0 .. p0 + n - 1 of dst [Z][dst_z / D][D] (bf16, D % 8 == 0)
__global__ void __launch_bounds__(256) kv_append_kernel(const bf16_t* __restrict__ src, long src_z,
                                                        bf16_t* __restrict__ dst, long dst_z, int p0, int n, int D,
                                                        long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;   // one 16-B chunk
  if (i >= total) return;
  const int per = D / 8;
  const long z = i / ((long)n * per);
  const long r = i - z * n * per;
  const int s = (int)(r / per), c = (int)(r - (long)s * per);
  *reinterpret_cast<uint4*>(dst + z * dst_z + (long)(p0 + s) * D + 8 * c) =
      *reinterpret_cast<const uint4*>(src + z * src_z + (long)s * D + 8 * c);
}
int launch_kv_append(const bf16_t* src, long src_z, bf16_t* dst, long dst_z, int Z, int p0, int n, int D,
                     hipStream_t st) {
  if (D % 8) return set_error("kv_append: head_dim %% 8");
  const long total = (long)Z * n * (D / 8);
  if (total <= 0) return 0;
  hipLaunchKernelGGL(kv_append_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, src, src_z, dst,
                     dst_z, p0, n, D, total);
  return hipGetLastError() == hipSuccess ? 0 : set_error("kv_append launch failed");
}

}  // namespace ptk

// ================================================================== stepwise decode (beam search)
// The pieces of ptk_gemma3_decode_prefill / _step (models.cpp): Stage 2's validation generate
// (Stage2/trainer.py:596-626: inputs_embeds = [projected image tokens | question], attention_mask with the padded
// question tokens 0, num_beams 3, do_sample, top_k 50, top_p 0.9) needs per-row prompt masks, the position ids HF
// derives from them (GenerationMixin._prepare_position_ids_for_generation: cumsum(mask) - 1, masked -> 0), and the
// cache rows re-ordered by the selected beams every step.

namespace ptk {

// prompt p = r / repeat -> decode row r: x rows r*Pp + i (i < P from src, else 0); key flag = (i < P) & mask[p][i]
__global__ void __launch_bounds__(256) dec_prompt_kernel(const float* __restrict__ src, long ld_b,
                                                         const int32_t* __restrict__ mask, long mask_ld, int repeat,
                                                         int P, int Pp, int H, float* __restrict__ x,
                                                         int32_t* __restrict__ kv) {
  const long row = blockIdx.x;
  const int r = (int)(row / Pp), i = (int)(row - (long)r * Pp), pr = r / repeat;
  const bool in = i < P;
  if (threadIdx.x == 0) kv[row] = in && (!mask || mask[(long)pr * mask_ld + i] != 0);
  float* xr = x + row * H;
  const float* sr = src + ((long)pr * ld_b + (in ? i : 0)) * H;
  for (int c = threadIdx.x * 4; c < H; c += 1024)
    *reinterpret_cast<float4*>(xr + c) = in ? *reinterpret_cast<const float4*>(sr + c) : make_float4(0, 0, 0, 0);
}

// one wave per decode row: position ids of the prompt slots (cumsum of the key flags - 1, 0 where masked), the
// row's slot-valid flags for the cache (slots < P), its valid count (the next position)
__global__ void __launch_bounds__(64) dec_positions_kernel(const int32_t* __restrict__ kv, int P, int Pp, int Smax,
                                                           int32_t* __restrict__ pos, int32_t* __restrict__ slot_ok,
                                                           int32_t* __restrict__ nvalid) {
  const int r = blockIdx.x, lane = threadIdx.x;
  int base = 0;
  for (int i0 = 0; i0 < Pp; i0 += 64) {
    const int i = i0 + lane;
    const int v = i < Pp ? kv[(long)r * Pp + i] : 0;
    const uint64_t m = __ballot(v != 0);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (i < Pp) pos[(long)r * Pp + i] = v ? base + before : 0;
    if (i < P) slot_ok[(long)r * Smax + i] = v;
    base += __popcll(m);
  }
  for (int i = P + lane; i < Smax; i += 64) slot_ok[(long)r * Smax + i] = 0;
  if (lane == 0) nvalid[r] = base;
}

// decode step t (slot p0 = P + t - 1): the new token's slot becomes valid, its position is the row's valid count
// + t - 1, and the key flags of cache slots [k_lo, k_lo + nk) (nk a multiple of 4, slots past p0 masked) are
// copied out contiguous for the attention call
__global__ void __launch_bounds__(256) dec_step_prep_kernel(int32_t* __restrict__ slot_ok, const int32_t* __restrict__ nvalid,
                                                            int Smax, int p0, int t, int k_lo, int nk,
                                                            int32_t* __restrict__ pos, int32_t* __restrict__ kmask) {
  const int r = blockIdx.x;
  const int32_t* so = slot_ok + (long)r * Smax;
  for (int j = threadIdx.x; j < nk; j += 256) {
    const int s = k_lo + j;
    kmask[(long)r * nk + j] = s < p0 ? so[s] : (s == p0 ? 1 : 0);
  }
  if (threadIdx.x == 0) {
    slot_ok[(long)r * Smax + p0] = 1;
    pos[r] = nvalid[r] + t - 1;
  }
}

// out row r = in row src[r] (16-B chunks; rows of `row_bytes`, a multiple of 16)
__global__ void __launch_bounds__(256) dec_gather_rows_kernel(const uint4* __restrict__ in, uint4* __restrict__ out,
                                                              const int32_t* __restrict__ src, long chunks_per_row,
                                                              long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long r = i / chunks_per_row, c = i - r * chunks_per_row;
  out[i] = in[(long)src[r] * chunks_per_row + c];
}

int launch_dec_prompt(const float* src, long ld_b, const int32_t* mask, long mask_ld, int repeat, int rows, int P,
                      int Pp, int H, float* x, int32_t* kv, hipStream_t st) {
  if (H % 4 || P > Pp || repeat < 1) return set_error("decode: prompt layout (H %% 4, P <= Pp, repeat >= 1)");
  hipLaunchKernelGGL(dec_prompt_kernel, dim3((unsigned)((long)rows * Pp)), dim3(256), 0, st, src, ld_b, mask, mask_ld,
                     repeat, P, Pp, H, x, kv);
  return hipGetLastError() == hipSuccess ? 0 : set_error("dec_prompt launch failed");
}
int launch_dec_positions(const int32_t* kv, int rows, int P, int Pp, int Smax, int32_t* pos, int32_t* slot_ok,
                         int32_t* nvalid, hipStream_t st) {
  hipLaunchKernelGGL(dec_positions_kernel, dim3((unsigned)rows), dim3(64), 0, st, kv, P, Pp, Smax, pos, slot_ok, nvalid);
  return hipGetLastError() == hipSuccess ? 0 : set_error("dec_positions launch failed");
}
int launch_dec_step_prep(int32_t* slot_ok, const int32_t* nvalid, int rows, int Smax, int p0, int t, int k_lo, int nk,
                         int32_t* pos, int32_t* kmask, hipStream_t st) {
  if (nk % 4 || k_lo + nk > Smax || p0 >= Smax) return set_error("decode: step layout (nk %d, k_lo %d, p0 %d)", nk, k_lo, p0);
  hipLaunchKernelGGL(dec_step_prep_kernel, dim3((unsigned)rows), dim3(256), 0, st, slot_ok, nvalid, Smax, p0, t, k_lo,
                     nk, pos, kmask);
  return hipGetLastError() == hipSuccess ? 0 : set_error("dec_step_prep launch failed");
}
int launch_dec_gather_rows(const void* in, void* out, const int32_t* src, int rows, long row_bytes, hipStream_t st) {
  if (row_bytes % 16) return set_error("decode: gathered rows must be multiples of 16 B");
  const long cpr = row_bytes / 16, total = cpr * rows;
  if (total <= 0) return 0;
  hipLaunchKernelGGL(dec_gather_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                     (const uint4*)in, (uint4*)out, src, cpr, total);
  return hipGetLastError() == hipSuccess ? 0 : set_error("dec_gather_rows launch failed");
}

__global__ void __launch_bounds__(256) dec_gather_i32_kernel(const int32_t* __restrict__ in, int32_t* __restrict__ out,
                                                              const int32_t* __restrict__ src, int rows) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r < rows) out[r] = in[src[r]];
}
__global__ void __launch_bounds__(256) dec_repeat_index_kernel(int32_t* __restrict__ src, int rows, int repeat) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r < rows) src[r] = r / repeat;
}
int launch_dec_gather_i32(const int32_t* in, int32_t* out, const int32_t* src, int rows, hipStream_t st) {
  hipLaunchKernelGGL(dec_gather_i32_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, in, out, src, rows);
  return hipGetLastError() == hipSuccess ? 0 : set_error("dec_gather_i32 launch failed");
}
int launch_dec_repeat_index(int32_t* src, int rows, int repeat, hipStream_t st) {
  hipLaunchKernelGGL(dec_repeat_index_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, src, rows, repeat);
  return hipGetLastError() == hipSuccess ? 0 : set_error("dec_repeat_index launch failed");
}

// ================================================================== token selection
// Four kernels pick the next token(s) of a bf16 logits row, one workgroup of SEL_T threads per row:
//   gen_sample_kernel / gen_sample_pen_kernel    one token per row (greedy / top-k / top-p draw): ptk_gemma3_generate
//   beam_cand_kernel / beam_cand_pen_kernel      a row's n_cand best continuations: ptk_beam_candidates
// each a composition of the block helpers below.  The helpers run on all SEL_T threads unless they say "thread 0",
// take the LDS arrays they work on as pointers, and name the barrier they end with.
constexpr int SEL_T = 1024;   // threads per row
constexpr int SEL_NW = SEL_T / 64;

// bf16 bits -> unsigned key with the order of the values (NaNs are not expected in logits)
PTK_DEV uint32_t bf_key(uint16_t u) { return (u & 0x8000u) ? (uint32_t)(~u & 0xffffu) : (uint32_t)(u | 0x8000u); }

// counter-based uniform in [0, 1) (splitmix64 of seed, step, row; 24 random bits)
PTK_DEV float gen_uniform(uint64_t seed, int step, int row) {
  uint64_t z = seed + 0x9e3779b97f4a7c15ull * (uint64_t)(1 + step) + 0xbf58476d1ce4e5b9ull * (uint64_t)(1 + row);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  z ^= z >> 31;
  return (float)(z >> 40) * (1.0f / 16777216.0f);
}

// f(i, u) for every element i < V of a bf16 row (u: the raw bits), each thread over elements in increasing index
// order: 16-B loads, four in flight per thread (the decode's per-token row passes are latency-bound otherwise:
// 2-byte loads one at a time measured ~0.8 ms per item at V = 262 144); the row must be 16-B aligned for the
// vector part (else everything goes through the scalar tail).  No barrier.
template <class F>
PTK_DEV void scan_row(const uint16_t* row, int V, F&& f) {
  const int tid = threadIdx.x;
  const int n8 = ((uintptr_t)row & 15) ? 0 : V / 8;
  const uint4* r4 = reinterpret_cast<const uint4*>(row);
  for (int c0 = tid; c0 < n8; c0 += 4 * SEL_T) {
    uint4 q[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = c0 + j * SEL_T;
      q[j] = c < n8 ? r4[c] : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = c0 + j * SEL_T;
      if (c < n8) {
        const uint32_t w[4] = {q[j].x, q[j].y, q[j].z, q[j].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          f(8 * c + 2 * e, (uint16_t)(w[e] & 0xffffu));
          f(8 * c + 2 * e + 1, (uint16_t)(w[e] >> 16));
        }
      }
    }
  }
  for (int i = 8 * n8 + tid; i < V; i += SEL_T) f(i, row[i]);
}

// ---- repetition penalty: the side list
// transformers RepetitionPenaltyLogitsProcessor (generation/logits_process.py): every DISTINCT token of a row's
// history (its own generated tokens so far) is penalised once, in fp32, x < 0 ? x * p : x / p -- on the raw logits
// before temperature / top-k / top-p when sampling (GenerationMixin._sample), on the log probs after log_softmax of
// the raw row in beam search (_beam_search; nothing is renormalised).  A penalised value is not a bf16, so it cannot
// pass through the 16-bit key selection: the history tokens of a row become a side list in LDS (token, raw bits), a
// V-bit LDS bitmap keeps them out of the bf16-keyed passes (their keys are subtracted from the radix histograms, and
// they are skipped where the passes collect), and the side list joins the kept list with its fp32 penalised scores.
// The kept set is then the kk largest (ties kept) of that union, selected in fp32 on the sorted LDS list: with p > 1
// history tokens leave the top set, with p < 1 up to n_hist of them enter it.  The plain kernels pass an empty side
// list (the launchers send p == 1 or an empty history to them).
constexpr int PEN_CAP = 1024;      // kk + n_hist at most (checked on the host before the launch; <= SEL_T: one
                                   // thread per history token)
static_assert(PEN_CAP <= SEL_T, "one thread per history token");
constexpr int PEN_VMAX = 294912;   // vocab at most: the bitmap takes V / 8 bytes of LDS (36 KiB here)
struct SideList {
  int n;                 // history length (0: no side list)
  const int* tok;        // [n] the token where it is the first of its value to arrive, else -1
  const uint16_t* bits;  // [n] its raw logit
  const uint32_t* bm;    // one bit per vocabulary entry, set for the tokens of the list (nullptr: no side list)
};
PTK_DEV float pen_apply(float x, float p) { return x < 0.f ? x * p : x / p; }
PTK_DEV bool side_member(const SideList& s, int i) { return s.bm && ((s.bm[i >> 5] >> (i & 31)) & 1u); }

// the row's side list from its history h[0 .. n_hist): a repeat or an id outside [0, V) gets token -1.  Ends with
// a barrier.
PTK_DEV SideList side_list_build(const int64_t* __restrict__ h, int n_hist, const uint16_t* row, int V, uint32_t* bm,
                                 int* h_tok, uint16_t* h_bits) {
  const int tid = threadIdx.x;
  for (int i = tid; i < (V + 31) / 32; i += SEL_T) bm[i] = 0;
  __syncthreads();
  if (tid < n_hist) {
    const long t = h[tid];
    int keep = -1;
    uint16_t u = 0;
    if (t >= 0 && t < V) {
      const uint32_t bit = 1u << (t & 31);
      if (!(atomicOr(&bm[t >> 5], bit) & bit)) { keep = (int)t; u = row[t]; }
    }
    h_tok[tid] = keep;
    h_bits[tid] = u;
  }
  __syncthreads();
  return SideList{n_hist, h_tok, h_bits, bm};
}

// ---- block reductions (redf / redi: SEL_NW words each; all end with a barrier, after which redf / redi are free)
// the maximum of (mx, mi) over the block, ties to the lowest index
PTK_DEV void block_argmax_first(float& mx, int& mi, float* redf, int* redi) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float ov = __shfl_xor(mx, o, 64);
    const int oi = __shfl_xor(mi, o, 64);
    if (ov > mx || (ov == mx && oi < mi)) { mx = ov; mi = oi; }
  }
  if (lane == 0) { redf[wave] = mx; redi[wave] = mi; }
  __syncthreads();
  mx = redf[0];
  mi = redi[0];
  for (int w = 1; w < SEL_NW; ++w)
    if (redf[w] > mx || (redf[w] == mx && redi[w] < mi)) { mx = redf[w]; mi = redi[w]; }
  __syncthreads();
}
// op over the block's values, in wave order (op: commutative, exact on the wave shuffles' pairing)
template <class Op>
PTK_DEV float block_reduce(float v, float* redf, Op&& op) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
  if (lane == 0) redf[wave] = v;
  __syncthreads();
  v = redf[0];
  for (int w = 1; w < SEL_NW; ++w) v = op(v, redf[w]);
  __syncthreads();
  return v;
}
// log-sum-exp of the raw row (fp32 over the bf16 logits): the log_softmax statistic
PTK_DEV float row_lse(const uint16_t* row, int V, float* redf) {
  float mx = -INFINITY;
  scan_row(row, V, [&](int, uint16_t u) { mx = fmaxf(mx, bf2f(u)); });
  mx = block_reduce(mx, redf, [](float a, float b) { return fmaxf(a, b); });
  float se = 0.f;
  scan_row(row, V, [&](int, uint16_t u) { se += __expf(bf2f(u) - mx); });
  return mx + __logf(block_reduce(se, redf, [](float a, float b) { return a + b; }));
}

// ---- the kept list
// key of the kk-th largest raw logit (kk < V) among the entries outside the side list: a two-pass radix select over
// the 16-bit keys (high byte, then low byte; the side list's keys leave each histogram again); fewer than kk such
// entries: 0 (all of them).  hist: 256 words, sel: 2.  Ends with a barrier.
PTK_DEV uint32_t radix_threshold(const uint16_t* row, int V, int kk, const SideList& side, uint32_t* hist,
                                 uint32_t* sel) {
  const int tid = threadIdx.x;
  uint32_t need = (uint32_t)kk, hi = 0, thr = 0;
  for (int pass = 0; pass < 2; ++pass) {
    for (int i = tid; i < 256; i += SEL_T) hist[i] = 0;
    __syncthreads();
    scan_row(row, V, [&](int, uint16_t u) {
      const uint32_t key = bf_key(u);
      if (pass == 0) atomicAdd(&hist[key >> 8], 1u);
      else if ((key >> 8) == hi) atomicAdd(&hist[key & 255u], 1u);
    });
    __syncthreads();
    if (side.n > 0) {   // (uniform)
      if (tid < side.n && side.tok[tid] >= 0) {
        const uint32_t key = bf_key(side.bits[tid]);
        if (pass == 0) atomicSub(&hist[key >> 8], 1u);
        else if ((key >> 8) == hi) atomicSub(&hist[key & 255u], 1u);
      }
      __syncthreads();
    }
    if (tid == 0) {
      uint32_t acc = 0;
      int bin = 255;
      for (; bin > 0; --bin) {
        if (acc + hist[bin] >= need) break;
        acc += hist[bin];
      }
      sel[0] = (uint32_t)bin;
      sel[1] = need > acc ? need - acc : 0u;   // how many of this bin's keys are still needed
    }
    __syncthreads();
    if (pass == 0) { hi = sel[0]; need = sel[1]; }
    else thr = (hi << 8) | sel[0];
    __syncthreads();
  }
  return thr;
}

// (score, token) of every entry outside the side list with key >= thr, and of every side-list entry, into ls / lt
// in arrival order; score(x, side) maps a raw logit to the entry's score.  Entries past `cap` are counted, not
// stored.  Returns the count (> cap: the list overflowed).  *cnt is written here only, so the count stays readable.
// Ends with a barrier.
template <class S>
PTK_DEV int collect_kept(const uint16_t* row, int V, uint32_t thr, const SideList& side, S&& score, float* ls,
                         int* lt, int* cnt, int cap) {
  const int tid = threadIdx.x;
  if (tid == 0) *cnt = 0;
  __syncthreads();
  scan_row(row, V, [&](int i, uint16_t u) {
    if (bf_key(u) >= thr && !side_member(side, i)) {
      const int slot = atomicAdd(cnt, 1);
      if (slot < cap) { ls[slot] = score(bf2f(u), false); lt[slot] = i; }
    }
  });
  if (tid < side.n && side.tok[tid] >= 0) {
    const int slot = atomicAdd(cnt, 1);
    if (slot < cap) { ls[slot] = score(bf2f(side.bits[tid]), true); lt[slot] = side.tok[tid]; }
  }
  __syncthreads();
  return *cnt;
}

// ls / lt [0, n) ascending by score, then token (bitonic; the arrays hold n rounded up to a power of two).  Ends
// with a barrier.
PTK_DEV void sort_kept(float* ls, int* lt, int n) {
  const int tid = threadIdx.x;
  int np2 = 1;
  while (np2 < n) np2 <<= 1;
  for (int i = n + tid; i < np2; i += SEL_T) { ls[i] = INFINITY; lt[i] = 0x7fffffff; }
  __syncthreads();
  for (int size = 2; size <= np2; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = tid; i < np2; i += SEL_T) {
        const int j = i ^ stride;
        if (j > i) {
          const bool up = (i & size) == 0;
          const float a = ls[i], c = ls[j];
          const bool gt = a > c || (a == c && lt[i] > lt[j]);
          if (gt == up) { ls[i] = c; ls[j] = a; const int tt = lt[i]; lt[i] = lt[j]; lt[j] = tt; }
        }
      }
      __syncthreads();
    }
}

// thread 0, sorted list: start of the kk largest, ties with the kk-th kept (TopKLogitsWarper: scores < the kk-th
// dropped; the plain kernels' radix threshold has done this already)
PTK_DEV int top_k_first(const float* ls, int n, int kk) {
  if (n <= kk) return 0;
  int lo = n - kk;
  const float kv = ls[lo];
  while (lo > 0 && ls[lo - 1] == kv) --lo;
  return lo;
}
// thread 0, sorted list [lo, n): TopPLogitsWarper -- the cumulative softmax from the smallest score up, entries with
// cumulative mass <= 1 - top_p dropped, the last min_keep kept.  Returns the start of what is left.
PTK_DEV int top_p_first(const float* ls, int n, int lo, float top_p, int min_keep) {
  if (!(top_p < 1.f)) return lo;
  const float top = ls[n - 1];
  float tot = 0.f;
  for (int i = lo; i < n; ++i) tot += __expf(ls[i] - top);
  float cum = 0.f;
  int first = lo;
  for (int i = lo; i < n; ++i) {
    cum += __expf(ls[i] - top);
    if (cum / tot <= 1.f - top_p) first = i + 1;
  }
  return min(first, max(lo, n - min_keep));
}
// thread 0, sorted list [first, n) of scores relative to the row maximum (<= 0): the token at uniform u by inverse
// CDF of softmax (sorted order: the same law as a draw in index order)
PTK_DEV int draw_sorted(const float* ls, const int* lt, int first, int n, float u) {
  float kept = 0.f;
  for (int i = first; i < n; ++i) kept += __expf(ls[i]);
  const float target = u * kept;
  float s = 0.f;
  for (int i = first; i < n; ++i) {
    s += __expf(ls[i]);
    if (target < s) return lt[i];
  }
  return lt[n - 1];
}
// the same draw without a list, in index order over the row's entries with key >= thr: the kept mass of a contiguous
// chunk per thread (prefix: SEL_T floats), a serial scan of the chunk sums, the chunk that holds the target.  Returns
// the token, or -1 where rounding left the target past the total.  Ends with a barrier.
PTK_DEV int draw_index_order(const uint16_t* row, int V, uint32_t thr, float mx, float inv_t, float u, float* prefix,
                             float* redf, int* redi) {
  const int tid = threadIdx.x;
  const int chunk = (V + SEL_T - 1) / SEL_T, c0 = tid * chunk, c1 = min(V, c0 + chunk);
  float part = 0.f;
  for (int i = c0; i < c1; ++i) {
    const uint16_t b = row[i];
    if (bf_key(b) >= thr) part += __expf((bf2f(b) - mx) * inv_t);
  }
  prefix[tid] = part;
  __syncthreads();
  if (tid == 0) {   // exclusive scan (1024 floats, once per token)
    float s = 0.f;
    for (int t = 0; t < SEL_T; ++t) { const float v = prefix[t]; prefix[t] = s; s += v; }
    redf[0] = s;
    redi[0] = -1;
  }
  __syncthreads();
  const float target = u * redf[0];
  const float lo = prefix[tid];
  if (lo <= target && target < lo + part) {
    float s = lo;
    int pick = -1, last = -1;
    for (int i = c0; i < c1; ++i) {
      const uint16_t b = row[i];
      if (bf_key(b) < thr) continue;
      last = i;
      s += __expf((bf2f(b) - mx) * inv_t);
      if (target < s) { pick = i; break; }
    }
    redi[0] = pick >= 0 ? pick : last;
  }
  __syncthreads();
  return redi[0];
}

PTK_DEV float bc_gumbel(uint64_t seed, int step, int row, int tok) {
  uint64_t z = seed ^ (0x9e3779b97f4a7c15ull * (uint64_t)(1 + step));
  z += 0xbf58476d1ce4e5b9ull * (uint64_t)(1 + row) + 0x94d049bb133111ebull * (uint64_t)(1 + tok);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  z ^= z >> 31;
  const float u = ((float)(z >> 40) + 0.5f) * (1.0f / 16777216.0f);   // (0, 1)
  return -__logf(-__logf(u));
}
// Decode row rowi's best n_cand (<= 32) of the list entries [first, n) into the scratch (selection key, accumulated
// score, token; token -2 on every entry when `bad`, -1 past the entries there were): ls becomes the accumulated
// score (+ the row's beam score bs), the key is that (+ Gumbel noise when sampling), and n_cand rounds of a block
// arg-max (ties: the lower token) take the largest, marking them taken in lt.  The first barrier comes after every
// thread has read its arguments, so `first` may come out of redi[0]; ends without one.
struct BestList {   // (LDS) the candidates taken so far, in the order taken
  float key[32], acc[32];
  int tok[32], n;
};
PTK_DEV void pick_candidates(float* ls, int* lt, int first, int n, float bs, int n_cand, int do_sample, uint64_t seed,
                             int step, int rowi, bool bad, float* redf, int* redi, BestList* best,
                             float* __restrict__ sc_key, float* __restrict__ sc_acc, int32_t* __restrict__ sc_tok) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) best->n = 0;
  for (int i = first + tid; i < n; i += SEL_T) ls[i] += bs;
  __syncthreads();
  for (int rnd = 0; rnd < n_cand; ++rnd) {
    float bk = -INFINITY;
    int bi = -1;
    for (int i = first + tid; i < n; i += SEL_T) {
      if (lt[i] < 0) continue;   // taken
      const float key = do_sample ? ls[i] + bc_gumbel(seed, step, rowi, lt[i]) : ls[i];
      if (key > bk || (key == bk && (bi < 0 || lt[i] < lt[bi]))) { bk = key; bi = i; }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const float ok = __shfl_xor(bk, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ok > bk || (ok == bk && oi >= 0 && (bi < 0 || lt[oi] < lt[bi]))) { bk = ok; bi = oi; }
    }
    if (lane == 0) { redf[wave] = bk; redi[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
      float k0 = redf[0];
      int i0 = redi[0];
      for (int w = 1; w < SEL_NW; ++w)
        if (redf[w] > k0 || (redf[w] == k0 && redi[w] >= 0 && (i0 < 0 || lt[redi[w]] < lt[i0]))) { k0 = redf[w]; i0 = redi[w]; }
      if (i0 >= 0 && k0 > -INFINITY) {
        best->key[best->n] = k0; best->acc[best->n] = ls[i0]; best->tok[best->n] = lt[i0];
        ++best->n;
        lt[i0] = -1;
      }
    }
    __syncthreads();
  }
  if (tid < n_cand) {
    const long o = (long)rowi * n_cand + tid;
    const bool ok = tid < best->n;
    sc_key[o] = ok ? best->key[tid] : -INFINITY;
    sc_acc[o] = ok ? best->acc[tid] : -INFINITY;
    sc_tok[o] = bad ? -2 : (ok ? best->tok[tid] : -1);
  }
}

// ---- one token per row
// HF generate's logits processors for do_sample, in GenerationMixin._sample's order: [repetition penalty on the raw
// logits,] temperature (z = x / T), top-k (every logit below the k-th largest dropped, ties kept; top_k <= 0 or >= V:
// all), top-p (min_tokens_to_keep 1), then one draw from softmax of what is left; greedy (do_sample == 0): the first
// index of the [penalised] maximum, as torch.argmax.  finished[b] != 0: the token is pad_id; a row whose token is
// eos_id becomes finished.  tok -> out[b * ld_out] and next[b].
constexpr int GS_LIST = 1024;    // kept entries the plain kernel sorts; more: the row falls back to its maximum
constexpr int PEN_LIST = 2048;   // ... the penalised kernels keep (PEN_CAP and the ties at the top-k boundary);
                                 // more: the status word makes the host call fail
__global__ void __launch_bounds__(SEL_T) gen_sample_kernel(const bf16_t* __restrict__ logits, long ld, int V,
                                                           int do_sample, int top_k, float temperature, float top_p,
                                                           uint64_t seed, int step, long eos_id, long pad_id,
                                                           int32_t* __restrict__ finished, int64_t* __restrict__ out,
                                                           long ld_out, int64_t* __restrict__ next) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const uint16_t* row = reinterpret_cast<const uint16_t*>(logits) + (long)b * ld;
  __shared__ uint32_t hist[256], sel[2];
  __shared__ float redf[SEL_NW], prefix[SEL_T], ls[GS_LIST];
  __shared__ int redi[SEL_NW], lt[GS_LIST], cnt;
  const SideList none{0, nullptr, nullptr, nullptr};
  const bool fin = finished[b] != 0;
  long tok = pad_id;
  if (!fin) {
    float mx = -INFINITY;
    int mi = 0x7fffffff;
    scan_row(row, V, [&](int i, uint16_t u) {
      const float v = bf2f(u);
      if (v > mx) { mx = v; mi = i; }
    });
    block_argmax_first(mx, mi, redf, redi);
    tok = mi;
    if (do_sample) {
      const int kk = (top_k > 0 && top_k < V) ? top_k : V;
      const uint32_t thr = kk < V ? radix_threshold(row, V, kk, none, hist, sel) : 0u;
      const float inv_t = 1.f / temperature, u = gen_uniform(seed, step, b);
      int pick;
      if (top_p < 1.f || (top_k > 0 && top_k <= GS_LIST / 2) || V <= GS_LIST) {
        // the kept set sorted in LDS; scores relative to the row max, which is in the list at +0
        const int c = collect_kept(row, V, thr, none, [&](float x, bool) { return (x - mx) * inv_t; }, ls, lt, &cnt,
                                   GS_LIST);
        const int n = min(c, GS_LIST);
        sort_kept(ls, lt, n);
        if (tid == 0) redi[0] = c > GS_LIST ? -1 : draw_sorted(ls, lt, top_p_first(ls, n, 0, top_p, 1), n, u);
        __syncthreads();
        pick = redi[0];
      } else {
        // top_p == 1 with a large or no top-k: no list, the draw in index order
        pick = draw_index_order(row, V, thr, mx, inv_t, u, prefix, redf, redi);
      }
      if (pick >= 0) tok = pick;   // (else an over-full list, or rounding past the total: the maximum)
    }
  }
  if (tid == 0) {
    out[(long)b * ld_out] = tok;
    next[b] = tok;
    if (!fin && tok == eos_id) finished[b] = 1;
  }
}

// the same with the repetition penalty: the history of row b is history[b * ld_hist + 0 .. n_hist).  top-k acts on
// the union of the radix-selected entries and the side list, in fp32 on the sorted list (top_k_first).
__global__ void __launch_bounds__(SEL_T) gen_sample_pen_kernel(const bf16_t* __restrict__ logits, long ld, int V,
                                                               int do_sample, int top_k, float temperature,
                                                               float top_p, uint64_t seed, int step, long eos_id,
                                                               long pad_id, int32_t* __restrict__ finished,
                                                               int64_t* __restrict__ out, long ld_out,
                                                               int64_t* __restrict__ next,
                                                               const int64_t* __restrict__ history, long ld_hist,
                                                               int n_hist, float pen, int32_t* __restrict__ status) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const uint16_t* row = reinterpret_cast<const uint16_t*>(logits) + (long)b * ld;
  extern __shared__ uint32_t pen_bm[];
  __shared__ int h_tok[PEN_CAP];
  __shared__ uint16_t h_bits[PEN_CAP];
  __shared__ uint32_t hist[256], sel[2];
  __shared__ float redf[SEL_NW], ls[PEN_LIST];
  __shared__ int redi[SEL_NW], lt[PEN_LIST], cnt;
  const bool fin = finished[b] != 0;
  long tok = pad_id;
  bool over = false;
  if (!fin) {
    const SideList side = side_list_build(history + (long)b * ld_hist, n_hist, row, V, pen_bm, h_tok, h_bits);
    // max (and its first index) of the penalised row: the entries outside the side list, then the side list
    float mx = -INFINITY;
    int mi = 0x7fffffff;
    scan_row(row, V, [&](int i, uint16_t u) {
      const float v = bf2f(u);
      if (v > mx && !side_member(side, i)) { mx = v; mi = i; }
    });
    if (tid < n_hist && h_tok[tid] >= 0) {
      const float v = pen_apply(bf2f(h_bits[tid]), pen);
      if (v > mx || (v == mx && h_tok[tid] < mi)) { mx = v; mi = h_tok[tid]; }
    }
    block_argmax_first(mx, mi, redf, redi);
    tok = mi;
    if (do_sample) {
      const int kk = (top_k > 0 && top_k < V) ? top_k : V;
      const uint32_t thr = kk < V ? radix_threshold(row, V, kk, side, hist, sel) : 0u;
      const float inv_t = 1.f / temperature;
      const int n = collect_kept(row, V, thr, side,
                                 [&](float x, bool s) { return ((s ? pen_apply(x, pen) : x) - mx) * inv_t; }, ls, lt,
                                 &cnt, PEN_LIST);
      over = n > PEN_LIST;
      tok = pad_id;   // an over-full list: the row stops with pad_id and the status word makes the host call fail
      if (!over) {
        sort_kept(ls, lt, n);
        if (tid == 0)
          redi[0] = draw_sorted(ls, lt, top_p_first(ls, n, top_k_first(ls, n, kk), top_p, 1), n,
                                gen_uniform(seed, step, b));
        __syncthreads();
        tok = redi[0];
      }
    }
  }
  if (tid == 0) {
    if (over) atomicOr(status, 1);
    out[(long)b * ld_out] = tok;
    next[b] = tok;
    if (!fin && (tok == eos_id || over)) finished[b] = 1;
  }
}

// ---- a row's beam candidates
// GenerationMixin._beam_search, one step (b, c of its loop: transformers/generation/utils.py _get_top_k_continuations):
// per decode row (batch item b, beam k) log_probs = log_softmax(fp32 logits) [, the repetition penalty on them]; with
// do_sample the warpers act on them in HF's order -- temperature (/T), top-k (keep >= the k-th largest, k =
// max(top_k, min_keep)), top-p (sort ascending, cumulative softmax, drop where <= 1 - top_p, keep the last min_keep)
// -- the rest -inf; + the beam's running score; then over the beams x vocab of item b:
//   do_sample: n_cand draws without replacement from softmax(accumulated) (torch.multinomial), taken as the
//              n_cand largest accumulated + Gumbel noise (the same distribution; order = draw order);
//   greedy:    the n_cand largest accumulated (torch.topk, descending).
// Out per item: tokens, beam (0..K-1) and the accumulated log prob (without the noise) of each candidate.
// One workgroup per decode row (item b = blockIdx / K, beam k = blockIdx % K): the row's best n_cand candidates
// into the scratch; beam_merge_kernel then takes each item's best n_cand over its K rows.
constexpr int BC_LIST = 1024;   // kept entries per row (top-k with ties) of the plain kernel; more -> token -2
__global__ void __launch_bounds__(SEL_T) beam_cand_kernel(const bf16_t* __restrict__ logits, long ld,
                                                          const float* __restrict__ beam_scores, int K, int V,
                                                          int do_sample, int top_k, float top_p, float temperature,
                                                          int min_keep, uint64_t seed, int step, int n_cand,
                                                          float* __restrict__ sc_key, float* __restrict__ sc_acc,
                                                          int32_t* __restrict__ sc_tok) {
  const int rowi = blockIdx.x, tid = threadIdx.x;
  __shared__ uint32_t hist[256], sel[2];
  __shared__ float redf[SEL_NW], ls[BC_LIST];   // ls / lt: the kept entries' processed log prob and token
  __shared__ int redi[SEL_NW], lt[BC_LIST], cnt;
  __shared__ BestList best;
  const SideList none{0, nullptr, nullptr, nullptr};
  const float inv_t = (do_sample && temperature > 0.f) ? 1.f / temperature : 1.f;
  const uint16_t* row = reinterpret_cast<const uint16_t*>(logits) + (long)rowi * ld;
  const float lse = row_lse(row, V, redf);
  // the kk largest logits (ties kept) -- log_softmax and /T preserve the order
  const int kk = do_sample ? (top_k > 0 ? max(top_k, min_keep) : V) : n_cand;
  const uint32_t thr = kk < V ? radix_threshold(row, V, kk, none, hist, sel) : 0u;
  const int c = collect_kept(row, V, thr, none, [&](float x, bool) { return (x - lse) * inv_t; }, ls, lt, &cnt,
                             BC_LIST);
  const int n = min(c, BC_LIST);
  const bool top_p_on = do_sample && top_p < 1.f;
  if (top_p_on) sort_kept(ls, lt, n);
  if (tid == 0) redi[0] = top_p_on ? top_p_first(ls, n, 0, top_p, min_keep) : 0;
  __syncthreads();
  pick_candidates(ls, lt, redi[0], n, beam_scores[rowi], n_cand, do_sample, seed, step, rowi, c > BC_LIST, redf, redi,
                  &best, sc_key, sc_acc, sc_tok);
}

// the same with the repetition penalty: the history of decode row r is history[r * ld_hist + 0 .. n_hist).  The
// penalty acts on the log probs of the RAW row; sampling takes top-k (ties kept) of the union in fp32 and then top-p
// on the sorted list, greedy needs neither (the n_cand rounds take the largest of the whole list).
__global__ void __launch_bounds__(SEL_T) beam_cand_pen_kernel(const bf16_t* __restrict__ logits, long ld,
                                                              const float* __restrict__ beam_scores, int K, int V,
                                                              int do_sample, int top_k, float top_p,
                                                              float temperature, int min_keep, uint64_t seed,
                                                              int step, int n_cand, float* __restrict__ sc_key,
                                                              float* __restrict__ sc_acc,
                                                              int32_t* __restrict__ sc_tok,
                                                              const int64_t* __restrict__ history, long ld_hist,
                                                              int n_hist, float pen, int32_t* __restrict__ status) {
  const int rowi = blockIdx.x, tid = threadIdx.x;
  extern __shared__ uint32_t pen_bm[];
  __shared__ int h_tok[PEN_CAP];
  __shared__ uint16_t h_bits[PEN_CAP];
  __shared__ uint32_t hist[256], sel[2];
  __shared__ float redf[SEL_NW], ls[PEN_LIST];
  __shared__ int redi[SEL_NW], lt[PEN_LIST], cnt;
  __shared__ BestList best;
  const float inv_t = (do_sample && temperature > 0.f) ? 1.f / temperature : 1.f;
  const uint16_t* row = reinterpret_cast<const uint16_t*>(logits) + (long)rowi * ld;
  const SideList side = side_list_build(history + (long)rowi * ld_hist, n_hist, row, V, pen_bm, h_tok, h_bits);
  const float lse = row_lse(row, V, redf);
  const int kk = do_sample ? (top_k > 0 ? max(top_k, min_keep) : V) : n_cand;
  const uint32_t thr = kk < V ? radix_threshold(row, V, kk, side, hist, sel) : 0u;
  const int c = collect_kept(row, V, thr, side,
                             [&](float x, bool s) { return (s ? pen_apply(x - lse, pen) : x - lse) * inv_t; }, ls, lt,
                             &cnt, PEN_LIST);
  const int n = min(c, PEN_LIST);
  const bool bad = c > PEN_LIST;
  if (bad && tid == 0) atomicOr(status, 1);
  if (do_sample) sort_kept(ls, lt, n);
  if (tid == 0) redi[0] = do_sample ? top_p_first(ls, n, top_k_first(ls, n, kk), top_p, min_keep) : 0;
  __syncthreads();
  pick_candidates(ls, lt, redi[0], n, beam_scores[rowi], n_cand, do_sample, seed, step, rowi, bad, redf, redi, &best,
                  sc_key, sc_acc, sc_tok);
}

// item b: the best n_cand over its K rows' lists (descending key; ties: the lower beam, then the lower token)
__global__ void __launch_bounds__(64) beam_merge_kernel(const float* __restrict__ sc_key,
                                                        const float* __restrict__ sc_acc,
                                                        const int32_t* __restrict__ sc_tok, int K, int n_cand,
                                                        int64_t* __restrict__ out_tok, int32_t* __restrict__ out_beam,
                                                        float* __restrict__ out_score) {
  const int b = blockIdx.x, lane = threadIdx.x;
  if (lane != 0) return;   // (K x n_cand <= 256 entries, once per item and step)
  const long base = (long)b * K * n_cand;
  bool bad = false;
  for (int i = 0; i < K * n_cand; ++i) bad |= sc_tok[base + i] == -2;
  int taken[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // next unread entry of each row's (descending) list
  for (int c = 0; c < n_cand; ++c) {
    int best = -1;
    float bk = -INFINITY;
    for (int k = 0; k < K; ++k) {
      if (taken[k] >= n_cand) continue;
      const long o = base + (long)k * n_cand + taken[k];
      if (sc_tok[o] < 0) continue;
      const float key = sc_key[o];
      if (best < 0 || key > bk) { bk = key; best = k; }   // (a tie keeps the lower beam)
    }
    const long out = (long)b * n_cand + c;
    if (best < 0 || bad) {
      out_tok[out] = -1; out_beam[out] = -1; out_score[out] = -INFINITY;
      continue;
    }
    const long o = base + (long)best * n_cand + taken[best];
    out_tok[out] = sc_tok[o]; out_beam[out] = best; out_score[out] = sc_acc[o];
    ++taken[best];
  }
}

// ---- host side
int pen_validate(const char* who, const PenArgs& pa) {
  if (!(pa.penalty > 0.f) || !std::isfinite(pa.penalty))
    return set_error("%s: repetition_penalty must be a finite float > 0 (got %g)", who, (double)pa.penalty);
  if (pa.n_hist < 0) return set_error("%s: n_hist %d < 0", who, pa.n_hist);
  if (pa.n_hist > 0 && !pa.history) return set_error("%s: history is NULL with n_hist %d", who, pa.n_hist);
  if (pa.ld_hist < pa.n_hist) return set_error("%s: history_ld %ld < n_hist %d", who, pa.ld_hist, pa.n_hist);
  return 0;
}
static int pen_capacity(const char* who, int kk, int n_hist, int V) {
  if ((long)kk + n_hist > PEN_CAP)
    return set_error("%s: repetition_penalty keeps top-k + history in LDS: %d + %d tokens exceed the limit of %d",
                     who, kk, n_hist, PEN_CAP);
  if (V > PEN_VMAX) return set_error("%s: repetition_penalty needs vocab <= %d (the history bitmap in LDS)", who, PEN_VMAX);
  return 0;
}
// the entries a step keeps ahead of top-p (the one definition of kk; the kernels compute the same)
static int gen_sample_kk(int V, int do_sample, int top_k) {
  return do_sample ? ((top_k > 0 && top_k < V) ? top_k : V) : 0;
}
static int beam_kk(int V, int do_sample, int top_k, int min_keep, int n_cand) {
  return std::min(V, do_sample ? (top_k > 0 ? std::max(top_k, min_keep) : V) : n_cand);
}
// Every host-side rule of one sampling step / one beam selection, penalised or not, with no device call: the
// launchers run them first, and so does an entry point that has device work of its own ahead of the launch.
int gen_sample_validate(const char* who, int V, int do_sample, int top_k, float temperature, float top_p,
                        const PenArgs& pa) {
  if (pen_validate(who, pa)) return -1;
  if (do_sample && !(temperature > 0.f)) return set_error("%s: temperature must be > 0 when sampling", who);
  if (do_sample && !(top_p > 0.f && top_p <= 1.f)) return set_error("%s: top_p must be in (0, 1]", who);
  if (pen_active(pa)) return pen_capacity(who, gen_sample_kk(V, do_sample, top_k), pa.n_hist, V);
  if (do_sample && top_p < 1.f && !(top_k > 0 && top_k <= GS_LIST / 2) && V > GS_LIST / 2)
    return set_error("%s: top_p < 1 needs 0 < top_k <= %d (the kept set is sorted in LDS)", who, GS_LIST / 2);
  return 0;
}
size_t beam_candidates_ws_bytes(int batch, int K, int n_cand) {
  return (size_t)batch * K * n_cand * 12 + 256;
}
int beam_candidates_validate(int batch, int K, int V, int do_sample, int top_k, float top_p, float temperature,
                             int min_keep, int n_cand, const void* ws, size_t ws_bytes, const PenArgs& pa) {
  const char* who = "beam_candidates";
  if (pen_validate(who, pa)) return -1;
  if (batch <= 0 || K <= 0 || K > 8 || V <= 0 || n_cand <= 0 || n_cand > 32)
    return set_error("beam_candidates: batch %d, beams %d (1..8), vocab %d, n_cand %d (1..32)", batch, K, V, n_cand);
  if (do_sample && !(temperature > 0.f)) return set_error("beam_candidates: temperature must be > 0 when sampling");
  if (do_sample && !(top_p > 0.f && top_p <= 1.f)) return set_error("beam_candidates: top_p must be in (0, 1]");
  if (pen_active(pa)) {
    if (pen_capacity(who, beam_kk(V, do_sample, top_k, min_keep, n_cand), pa.n_hist, V)) return -1;
  } else if (do_sample && !(top_k > 0 && top_k <= BC_LIST / 2) && V > BC_LIST / 2) {
    return set_error("beam_candidates: sampling needs 0 < top_k <= %d (the kept set lives in LDS)", BC_LIST / 2);
  }
  // (a penalised call keeps its status word in the 256 bytes behind the unpenalised workspace)
  const size_t need = beam_candidates_ws_bytes(batch, K, n_cand) + (pen_active(pa) ? 256 : 0);
  if (!ws || ws_bytes < need) return set_error("beam_candidates: workspace too small (%zu bytes needed)", need);
  return 0;
}
int pen_status_check(const char* who, int32_t* status, hipStream_t st) {
  int32_t h = 0;
  if (hipMemcpyAsync(&h, status, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return set_error("%s: reading the repetition-penalty status failed", who);
  if (h) return set_error("%s: more than %d entries to keep for one row (ties at the top-k boundary)", who, PEN_LIST);
  return 0;
}
static size_t pen_bitmap_bytes(int V) { return (size_t)((V + 31) / 32) * 4; }

int launch_gen_sample(const bf16_t* logits, long ld, int B, int V, int do_sample, int top_k, float temperature,
                      float top_p, uint64_t seed, int step, long eos_id, long pad_id, int32_t* finished, int64_t* out,
                      long ld_out, int64_t* next, const PenArgs& pa, hipStream_t st) {
  if (gen_sample_validate("generate", V, do_sample, top_k, temperature, top_p, pa)) return -1;
  if (!do_sample) top_p = 1.f;
  if (!pen_active(pa)) {
    hipLaunchKernelGGL(gen_sample_kernel, dim3((unsigned)B), dim3(SEL_T), 0, st, logits, ld, V, do_sample, top_k,
                       temperature, top_p, seed, step, eos_id, pad_id, finished, out, ld_out, next);
    return hipGetLastError() == hipSuccess ? 0 : set_error("gen_sample launch failed");
  }
  if (!pa.status) return set_error("generate: repetition_penalty needs a status word");
  hipLaunchKernelGGL(gen_sample_pen_kernel, dim3((unsigned)B), dim3(SEL_T), pen_bitmap_bytes(V), st, logits, ld, V,
                     do_sample, top_k, temperature, top_p, seed, step, eos_id, pad_id, finished, out, ld_out, next,
                     pa.history, pa.ld_hist, pa.n_hist, pa.penalty, pa.status);
  return hipGetLastError() == hipSuccess ? 0 : set_error("gen_sample_pen launch failed");
}

int launch_beam_candidates(const bf16_t* logits, long ld, const float* beam_scores, int batch, int K, int V,
                           int do_sample, int top_k, float top_p, float temperature, int min_keep, uint64_t seed,
                           int step, int n_cand, int64_t* tok, int32_t* beam, float* score, void* ws,
                           size_t ws_bytes, const PenArgs& pa, hipStream_t st) {
  if (beam_candidates_validate(batch, K, V, do_sample, top_k, top_p, temperature, min_keep, n_cand, ws, ws_bytes, pa))
    return -1;
  if (pen_active(pa) && !pa.status) return set_error("beam_candidates: repetition_penalty needs a status word");
  const long nr = (long)batch * K * n_cand;
  float* sk = (float*)ws;
  float* sa = sk + nr;
  int32_t* stok = (int32_t*)(sa + nr);
  const dim3 grid((unsigned)(batch * K));
  if (pen_active(pa))
    hipLaunchKernelGGL(beam_cand_pen_kernel, grid, dim3(SEL_T), pen_bitmap_bytes(V), st, logits, ld, beam_scores, K, V,
                       do_sample, top_k, top_p, temperature, min_keep, seed, step, n_cand, sk, sa, stok, pa.history,
                       pa.ld_hist, pa.n_hist, pa.penalty, pa.status);
  else
    hipLaunchKernelGGL(beam_cand_kernel, grid, dim3(SEL_T), 0, st, logits, ld, beam_scores, K, V, do_sample, top_k,
                       top_p, temperature, min_keep, seed, step, n_cand, sk, sa, stok);
  if (hipGetLastError() != hipSuccess)
    return set_error(pen_active(pa) ? "beam_candidates_pen launch failed" : "beam_candidates launch failed");
  hipLaunchKernelGGL(beam_merge_kernel, dim3((unsigned)batch), dim3(64), 0, st, sk, sa, stok, K, n_cand, tok, beam,
                     score);
  return hipGetLastError() == hipSuccess ? 0 : set_error("beam_merge launch failed");
}


}  // namespace ptk
