// C-ABI entry points: error reporting, primitive ops, projector, optimizer.
// Model-level orchestration (SigLIP, Gemma3) lives in models.cpp.
#include <stdarg.h>
#include <stdio.h>

#include "../../include/ptk.h"
#include "ptk_internal.h"

namespace ptk {

static thread_local char g_err[512] = "";

int set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return -1;
}

RowMap to_map(ptk_rowmap m) { return RowMap{m.g, m.skip, (long)m.gs, (long)m.off}; }

GemmArgs to_args(const ptk_gemm_desc* d) {
  GemmArgs a;
  a.A = (const bf16_t*)d->A; a.B = (const bf16_t*)d->B; a.C = d->C;
  a.M = d->M; a.N = d->N; a.K = d->K;
  a.lda = d->lda; a.ldb = d->ldb; a.ldc = d->ldc;
  a.zin = d->batch_inner > 0 ? d->batch_inner : 1;
  a.sA0 = d->sA0; a.sA1 = d->sA1; a.sB0 = d->sB0; a.sB1 = d->sB1; a.sC0 = d->sC0; a.sC1 = d->sC1;
  a.alpha = d->alpha;
  a.bias = d->bias; a.rowadd = d->rowadd; a.rowadd_period = d->rowadd_period > 0 ? d->rowadd_period : 1;
  a.ld_rowadd = d->ld_rowadd; a.resid = d->resid; a.ld_resid = d->ld_resid;
  a.aux = (bf16_t*)d->aux; a.aux2 = (bf16_t*)d->aux2; a.ld_aux = d->ld_aux;
  a.aux_in = (const bf16_t*)d->aux_in; a.aux_in2 = (const bf16_t*)d->aux_in2; a.ld_aux_in = d->ld_aux_in;
  a.amap = to_map(d->amap); a.cmap = to_map(d->cmap);
  a.resid16 = (const bf16_t*)d->resid16; a.ld_resid16 = d->ld_resid16; a.bf16_linear = d->bf16_linear;
  a.tail_ws = d->tail_ws;
  a.B_kt = (const bf16_t*)d->B_kt;
  a.a_kt = d->A_kt; a.c_kt = d->C_kt; a.aux_kt = d->aux_kt; a.aux_in_kt = d->aux_in_kt;
  return a;
}

// compute units of the current device: the library's one cache (256 when no device answers)
int device_cus() {
  static int n = 0;
  if (n == 0) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0)
      n = v;
    else
      n = 256;
  }
  return n;
}

}  // namespace ptk

using namespace ptk;
#define ST ((hipStream_t)stream)

extern "C" {

int ptk_abi_version(void) { return PTK_ABI_VERSION; }
const char* ptk_last_error(void) { return g_err; }

int ptk_gemm(const ptk_gemm_desc* d, void* stream) {
  if (!d) return set_error("ptk_gemm: null desc");
  if (d->act == PTK_ACT_GEGLU && (d->N % 32)) return set_error("ptk_gemm: GEGLU needs N %% 32 == 0");
  if (d->rowadd && d->rowadd_period <= 0)   // (to_args would make it 1)
    return set_error("ptk_gemm: rowadd_period %d must be positive", d->rowadd_period);
  return launch_gemm(to_args(d), d->act, d->out, d->batch > 0 ? d->batch : 1, ST);
}

size_t ptk_gemm_tail_scratch_bytes(void) { return p8_tail_scratch_bytes(); }
int ptk_gemm_tail_split(const ptk_gemm_desc* d) {
  if (!d) return set_error("ptk_gemm_tail_split: null desc");
  // the planner's tail plan over the descriptor's or the scope's scratch, without launch_gemm's M / N / batch gates
  return p8_tail_plan(to_args(d), d->act, d->out, gemm_plan_env()).gsplit;
}
// the planner's answers under the current force mode, with the descriptor's tail_ws as the only scratch (no
// model-level scope), on a device of ncu compute units: nothing is launched, so they hold without a GPU
static GemmPlanEnv test_plan_env(int ncu) {
  GemmPlanEnv e = gemm_plan_env();
  e.ncu = ncu;
  e.tail_scope = nullptr;
  return e;
}
int ptk_gemm_plan(const ptk_gemm_desc* d, int ncu, int* path, int* tile_rows, int* tail_split) {
  if (!d || ncu <= 0) return set_error("ptk_gemm_plan: null desc or ncu <= 0");
  const GemmPlan p = gemm_plan(to_args(d), d->act, d->out, d->batch > 0 ? d->batch : 1, test_plan_env(ncu));
  if (path) *path = p.path;
  if (tile_rows) *tile_rows = p.tm;
  if (tail_split) *tail_split = p.tail.gsplit;
  return 0;
}
int ptk_gemm_split_plan(const ptk_gemm_desc* d, int ncu, int64_t part_floats, int* slices, int* kc, int* rem,
                        int* tail_ws) {
  if (!d || ncu <= 0) return set_error("ptk_gemm_split_plan: null desc or ncu <= 0");
  const GemmSplitPlan s = gemm_split_plan(to_args(d), d->out, (long)part_floats, test_plan_env(ncu));
  if (slices) *slices = s.slices;
  if (kc) *kc = s.kc;
  if (rem) *rem = s.rem;
  if (tail_ws) *tail_ws = s.tail_ws ? 1 : 0;
  return 0;
}

size_t ptk_gemm_skinny_part_bytes(int M, int N, int K) { return skinny_part_bytes(M, N, K); }
int ptk_gemm_skinny(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int M, int N, int K,
                    int act, void* part, size_t part_bytes, void* stream) {
  if (!A || !B || !C) return set_error("ptk_gemm_skinny: NULL operand");
  return launch_gemm_skinny((const bf16_t*)A, (long)lda, (const bf16_t*)B, (long)ldb, (bf16_t*)C, (long)ldc, M, N, K,
                            act, (float*)part, part_bytes, (hipStream_t)stream);
}

int64_t ptk_layernorm_bwd_partial_floats(int rows, int cols) {
  return rows > 0 && cols > 0 ? (int64_t)layernorm_bwd_partial_floats(rows, cols) : 0;
}
int ptk_layernorm_bwd_bf16(const void* x, const float* w, const void* dy, const void* dacc, void* dx, int rows,
                           int cols, float eps, void* dw, void* db, float* partial, int64_t part_floats,
                           void* stream) {
  return launch_layernorm_bwd_bf16((const bf16_t*)x, w, (const bf16_t*)dy, (const bf16_t*)dacc, (bf16_t*)dx, rows,
                                   cols, eps, (bf16_t*)dw, (bf16_t*)db, partial, (long)part_floats, ST);
}
int ptk_gelu_tanh_bwd_bf16(const void* dg, const void* pre, void* dpre, int64_t rows, int cols, void* stream) {
  return launch_gelu_tanh_bwd_bf16((const bf16_t*)dg, (const bf16_t*)pre, (bf16_t*)dpre, (long)rows, cols, ST);
}
int ptk_colsum_bf16_acc(const void* x, int rows, int cols, void* grad, float* partial, int64_t part_floats,
                        void* stream) {
  if (!x || !grad || !partial) return set_error("colsum_bf16_acc: null argument");
  return launch_colsum_bf16_acc((const bf16_t*)x, rows, cols, (bf16_t*)grad, partial, (long)part_floats, ST);
}
int ptk_pos_grad_bf16(const void* dh0, int batch, int num_patches, int hidden, void* dpos, void* stream) {
  return launch_pos_grad_bf16((const bf16_t*)dh0, batch, num_patches, hidden, (bf16_t*)dpos, ST);
}

int ptk_layernorm(const float* x, const float* w, const float* b, void* y, int rows, int cols, float eps,
                  void* stream) {
  return launch_layernorm(x, w, b, (bf16_t*)y, rows, cols, eps, ST);
}

int ptk_rmsnorm(const float* x, const float* w, void* y, float* rstd, int rows, int cols, float eps, void* stream) {
  return launch_rmsnorm_fwd(x, cols, RowMap{0, 0, 0, 0}, w, (bf16_t*)y, rstd, rows, cols, eps, ST);
}

int ptk_rmsnorm_bwd(const float* x, const float* w, const float* rstd, const float* dn, const float* dacc, float* dx,
                    int rows, int cols, void* stream) {
  return launch_rmsnorm_bwd_f32(x, w, rstd, dn, dacc, dx, rows, cols, ST);
}

// ---- unit-test surface of the Gemma3 norm kernels and the norm weight-grad block: every argument is checked
// before any device call, then the launcher the model calls runs unchanged
static int norm_cols_ok(const char* who, int cols) {
  if (cols <= 0 || cols % 4 || cols > 3072) return set_error("%s: cols %d (multiple of 4, <= 3072)", who, cols);
  return 0;
}
// the norm kernels do not drop rows: a map with skip would index row -1
static int map_ok(const char* who, ptk_rowmap m) {
  if (m.g < 0 || m.skip != 0 || m.off < 0 || (m.g > 0 && m.gs < 0))
    return set_error("%s: row map {g %d, skip %d, gs %lld, off %lld} unsupported", who, m.g, m.skip, (long long)m.gs,
                     (long long)m.off);
  return 0;
}

int ptk_residual_norm_fwd(const void* t, const float* xi, const float* w_post, const float* w_next, float* xo, void* n,
                          float* rstd_t, float* rstd_x, int rows, int cols, float eps, void* stream) {
  if (norm_cols_ok("residual_norm_fwd", cols)) return -1;
  if (rows <= 0) return 0;
  if (!t || !xi || !w_post || !xo || !rstd_t || (w_next && (!n || !rstd_x)))
    return set_error("residual_norm_fwd: NULL argument");
  return launch_residual_norm_fwd((const bf16_t*)t, xi, w_post, w_next, xo, (bf16_t*)n, rstd_t, rstd_x, rows, cols, eps,
                                  ST);
}
int ptk_post_norm_bwd(const float* dR, const void* t, const float* w, const float* rstd_t, void* dt, int rows,
                      int cols, void* stream) {
  if (norm_cols_ok("post_norm_bwd", cols)) return -1;
  if (rows <= 0) return 0;
  if (!dR || !t || !w || !rstd_t || !dt) return set_error("post_norm_bwd: NULL argument");
  return launch_post_norm_bwd(dR, (const bf16_t*)t, w, rstd_t, (bf16_t*)dt, rows, cols, ST);
}
int ptk_rmsnorm_bwd_bdn(const float* x, const float* w, const float* rstd, const void* dn, const float* dacc,
                        float* dx, int rows, int cols, void* stream) {
  if (norm_cols_ok("rmsnorm_bwd_bdn", cols)) return -1;
  if (rows <= 0) return 0;
  if (!x || !w || !rstd || !dn || !dx) return set_error("rmsnorm_bwd_bdn: NULL argument");
  return launch_rmsnorm_bwd_bdn(x, w, rstd, (const bf16_t*)dn, dacc, dx, rows, cols, ST);
}
int ptk_rmsnorm_mapped(const float* x, int64_t ldx, ptk_rowmap xmap, const float* w, void* y, float* rstd, int rows,
                       int cols, float eps, void* stream) {
  if (norm_cols_ok("rmsnorm_mapped", cols) || map_ok("rmsnorm_mapped", xmap)) return -1;
  if (ldx < cols || ldx % 4) return set_error("rmsnorm_mapped: ldx %lld (>= cols %d, multiple of 4)", (long long)ldx, cols);
  if (rows <= 0) return 0;
  if (!x || !w || !y) return set_error("rmsnorm_mapped: NULL argument");
  return launch_rmsnorm_fwd(x, (long)ldx, to_map(xmap), w, (bf16_t*)y, rstd, rows, cols, eps, ST);
}
int ptk_rmsnorm_bwd_scatter(const float* x, ptk_rowmap xmap, const float* w, const float* rstd, const float* dn,
                            float* dR, int rows, int cols, void* stream) {
  if (norm_cols_ok("rmsnorm_bwd_scatter", cols) || map_ok("rmsnorm_bwd_scatter", xmap)) return -1;
  if (rows <= 0) return 0;
  if (!x || !w || !rstd || !dn || !dR) return set_error("rmsnorm_bwd_scatter: NULL argument");
  return launch_rmsnorm_bwd_scatter(x, to_map(xmap), w, rstd, dn, dR, rows, cols, ST);
}

// the surface takes at most 2^20 rows (the launchers' int partial sizes stay far below 2^31)
constexpr int kSurfaceMaxRows = 1 << 20;
int64_t ptk_rms_wgrad_partial_floats(int rows, int cols) {
  if (rows > kSurfaceMaxRows || cols > 4096) return -1;
  return rows > 0 && cols > 0 ? (int64_t)rms_wgrad_partial_floats(rows, cols) : 0;
}
int ptk_rms_wgrad(const void* x, int x_bf16, int64_t ldx, ptk_rowmap xmap, const float* rstd, const void* dy,
                  int dy_bf16, int64_t lddy, int dy_round, int rows, int cols, void* grad, float* partial,
                  int64_t part_floats, void* stream) {
  if (cols <= 0 || cols % 4 || cols > 4096) return set_error("rms_wgrad: cols %d (multiple of 4, <= 4096)", cols);
  if (map_ok("rms_wgrad", xmap)) return -1;
  if (ldx < cols || ldx % 4 || lddy < cols || lddy % 4)
    return set_error("rms_wgrad: ldx %lld / lddy %lld (>= cols %d, multiples of 4)", (long long)ldx, (long long)lddy,
                     cols);
  if (x_bf16 && dy_bf16) return set_error("rms_wgrad: x bf16 with dy bf16 is not instantiated");
  if (dy_bf16 && dy_round) return set_error("rms_wgrad: dy_round with a bf16 dy");
  if (rows > kSurfaceMaxRows) return set_error("rms_wgrad: %d rows (max %d)", rows, kSurfaceMaxRows);
  if (rows <= 0) return 0;
  if (!x || !rstd || !dy || !grad || !partial) return set_error("rms_wgrad: NULL argument");
  if (part_floats < ptk_rms_wgrad_partial_floats(rows, cols))
    return set_error("rms_wgrad: partial %lld floats < %lld", (long long)part_floats,
                     (long long)ptk_rms_wgrad_partial_floats(rows, cols));
  const RowMap m = to_map(xmap);
  if (x_bf16)
    return launch_rms_wgrad_bx((const bf16_t*)x, (long)ldx, m, rstd, (const float*)dy, (long)lddy, dy_round != 0, rows,
                               cols, (bf16_t*)grad, partial, ST);
  if (dy_bf16)
    return launch_rms_wgrad_bdy((const float*)x, (long)ldx, m, rstd, (const bf16_t*)dy, (long)lddy, rows, cols,
                                (bf16_t*)grad, partial, ST);
  return launch_rms_wgrad((const float*)x, (long)ldx, m, rstd, (const float*)dy, (long)lddy, dy_round != 0, rows, cols,
                          (bf16_t*)grad, partial, ST);
}
int64_t ptk_rms_wgrad_finish_floats(int nblk, int cols) {
  if (nblk > (1 << 18) || cols > 4096) return -1;
  return nblk > 0 && cols > 0 ? (int64_t)rms_wgrad_finish_floats(nblk, cols) : 0;
}
int ptk_rms_wgrad_finish(float* partial, int nblk, int cols, void* grad, int64_t part_floats, void* stream) {
  if (cols <= 0 || cols > 4096) return set_error("rms_wgrad_finish: cols %d (1 .. 4096)", cols);
  if (nblk > (1 << 18)) return set_error("rms_wgrad_finish: %d partial rows (max 262144)", nblk);
  if (nblk <= 0) return 0;
  if (!partial || !grad) return set_error("rms_wgrad_finish: NULL argument");
  if (part_floats < ptk_rms_wgrad_finish_floats(nblk, cols))
    return set_error("rms_wgrad_finish: partial %lld floats < %lld", (long long)part_floats,
                     (long long)ptk_rms_wgrad_finish_floats(nblk, cols));
  return launch_rms_wgrad_finish(partial, nblk, cols, (bf16_t*)grad, ST);
}
int64_t ptk_qknorm_wgrad_partial_floats(int64_t rows, int head_dim) {
  if (rows > kSurfaceMaxRows || head_dim > 256) return -1;
  return rows > 0 && head_dim > 0 ? (int64_t)qknorm_wgrad_partial_floats((long)rows, head_dim) : 0;
}
int ptk_qknorm_wgrad(const void* qkv, const float* cos_t, const float* sin_t, int batch, int seq, int heads,
                     int kv_heads, int head_dim, const float* rstd_q, const float* rstd_k, const void* dQ,
                     const void* dK, void* gq, void* gk, float* partial, int64_t part_floats, void* stream) {
  if (head_dim <= 0 || head_dim > 256 || head_dim % 8)
    return set_error("qknorm_wgrad: head_dim %d (multiple of 8, <= 256)", head_dim);
  if (heads <= 0 || kv_heads <= 0 || heads % kv_heads)
    return set_error("qknorm_wgrad: heads %d / kv_heads %d", heads, kv_heads);
  if (batch < 0 || seq < 0 || (int64_t)batch * seq > kSurfaceMaxRows)
    return set_error("qknorm_wgrad: batch %d x seq %d", batch, seq);
  const int64_t M = (int64_t)batch * seq;
  if (M == 0) return 0;
  if (!qkv || !cos_t || !sin_t || !rstd_q || !rstd_k || !dQ || !dK || !gq || !gk || !partial)
    return set_error("qknorm_wgrad: NULL argument");
  if (part_floats < ptk_qknorm_wgrad_partial_floats(M, head_dim))
    return set_error("qknorm_wgrad: partial %lld floats < %lld", (long long)part_floats,
                     (long long)ptk_qknorm_wgrad_partial_floats(M, head_dim));
  const AttnShape sh{batch, seq, heads, kv_heads, head_dim};
  return launch_qknorm_wgrad((const bf16_t*)qkv, cos_t, sin_t, sh, rstd_q, rstd_k, (const bf16_t*)dQ, (const bf16_t*)dK,
                             (bf16_t*)gq, (bf16_t*)gk, partial, ST);
}

int ptk_qknorm_rope_fwd(const void* qkv, const float* q_norm_w, const float* k_norm_w, const float* cos_t,
                        const float* sin_t, int batch, int seq, int heads, int kv_heads, int head_dim, float eps,
                        void* Q, void* K, void* V, float* rstd_q, float* rstd_k, void* stream) {
  const AttnShape sh{batch, seq, heads, kv_heads, head_dim};
  return launch_qknorm_rope_fwd((const bf16_t*)qkv, q_norm_w, k_norm_w, cos_t, sin_t, sh, eps, (bf16_t*)Q,
                                (bf16_t*)K, (bf16_t*)V, rstd_q, rstd_k, ST);
}
int ptk_qknorm_rope_bwd(const void* qkv, const float* q_norm_w, const float* k_norm_w, const float* cos_t,
                        const float* sin_t, int batch, int seq, int heads, int kv_heads, int head_dim,
                        const float* rstd_q, const float* rstd_k, const void* dQ, const void* dK, const void* dV,
                        void* dqkv, void* stream) {
  const AttnShape sh{batch, seq, heads, kv_heads, head_dim};
  return launch_qknorm_rope_bwd((const bf16_t*)qkv, q_norm_w, k_norm_w, cos_t, sin_t, sh, rstd_q, rstd_k,
                                (const bf16_t*)dQ, (const bf16_t*)dK, (const bf16_t*)dV, (bf16_t*)dqkv, ST);
}
int ptk_softmax(const float* S, void* P, int nz, int rows, int cols, int64_t ld, int rows_per_batch, int qdiv,
                int zdiv, int causal, int window, const int32_t* key_valid, int key_len, void* stream) {
  MaskSpec m{rows_per_batch > 0 ? rows_per_batch : rows, qdiv > 0 ? qdiv : 1, zdiv > 0 ? zdiv : 1, causal, window,
             key_valid, key_len};
  return launch_softmax_fwd(S, (bf16_t*)P, nz, rows, cols, ld, m, ST);
}

int ptk_cross_entropy(void* logits, int64_t ld, int rows, int vocab, const int64_t* targets, float* row_loss,
                      const float* gscale, void* stream) {
  return launch_ce_fwd_bwd((bf16_t*)logits, ld, rows, vocab, targets, row_loss, gscale, ST);
}

// ---- unit-test surface of the loss head (the lm_head GEMM's softmax statistics, the CE pass that reads them, the
// valid-label count and the loss mean): every argument is checked before any device call, then the launcher the
// model calls runs unchanged
int ptk_gemm_row_stats(const ptk_gemm_desc* d, float* stats, int64_t ld_stats, void* stream) {
  if (!d) return set_error("ptk_gemm_row_stats: null desc");
  if (!stats) return set_error("ptk_gemm_row_stats: NULL stats");
  if (!d->A || !d->B || !d->C) return set_error("ptk_gemm_row_stats: NULL operand (A, B or C)");
  GemmArgs a = to_args(d);
  a.row_stats = stats;
  a.ld_stats = (long)ld_stats;
  return launch_gemm(a, d->act, d->out, d->batch > 0 ? d->batch : 1, ST);   // (row_stats_check: the refusals)
}
int ptk_cross_entropy_stats(void* logits, int64_t ld, int rows, int vocab, const float* stats, int64_t ld_stats,
                            const int64_t* targets, float* row_loss, const float* gscale, void* stream) {
  if (vocab <= 0 || vocab % 64) return set_error("cross_entropy_stats: vocab %d must be a positive multiple of 64", vocab);
  if (ld % 8 || ld < vocab)
    return set_error("cross_entropy_stats: ld %lld (>= vocab %d, a multiple of 8)", (long long)ld, vocab);
  if (ld_stats < 2LL * (vocab / 64))
    return set_error("cross_entropy_stats: ld_stats %lld < 2 * vocab / 64 = %d", (long long)ld_stats, 2 * (vocab / 64));
  if (rows <= 0) return 0;
  if (!logits || !stats || !targets || !row_loss || !gscale) return set_error("cross_entropy_stats: NULL argument");
  if (((uintptr_t)logits & 15) || ((uintptr_t)stats & 7) || (ld_stats & 1))
    return set_error("cross_entropy_stats: logits must be 16-byte aligned, stats 8-byte aligned with an even ld_stats");
  return launch_ce_stats_fwd_bwd((bf16_t*)logits, (long)ld, rows, vocab, stats, (long)ld_stats, targets, row_loss,
                                 gscale, ST);
}
int ptk_count_valid(const int64_t* labels, int n, float loss_scale, float* gscale, float* count, void* stream) {
  if (!gscale || !count) return set_error("count_valid: NULL gscale / count");
  if (n > 0 && !labels) return set_error("count_valid: NULL labels");
  return launch_count_valid(labels, n > 0 ? n : 0, loss_scale, gscale, count, ST);
}
int ptk_loss_reduce(const float* row_loss, int rows, const float* count, float* loss, void* stream) {
  if (!count || !loss) return set_error("loss_reduce: NULL count / loss");
  if (rows > 0 && !row_loss) return set_error("loss_reduce: NULL row_loss");
  return launch_loss_reduce(row_loss, rows > 0 ? rows : 0, count, loss, ST);
}

int ptk_transpose_bf16(const void* in, int64_t ld_in, void* out, int64_t ld_out, int nz, int64_t s_in, int64_t s_out,
                       int rows, int cols, int rows_pad, void* stream) {
  return launch_transpose((const bf16_t*)in, ld_in, s_in, 0, 1, (bf16_t*)out, ld_out, s_out, 0, nz, rows, cols,
                          rows_pad, ST);
}

int ptk_transpose_rows_bf16(const void* in, int64_t ld_in, int map_g, int64_t map_gs, int64_t map_off, int rows,
                            int cols, void* out, int64_t ld_out, int rows_pad, void* stream) {
  const RowMap m{map_g, 0, map_gs, map_off};
  return launch_transpose_rows((const bf16_t*)in, ld_in, m, rows, cols, (bf16_t*)out, ld_out, rows_pad, ST);
}

int64_t ptk_kstep_tile_offset(int64_t row, int64_t k, int64_t K) { return kstep_tile_offset(row, k, K); }
int ptk_pack_kstep_tiles_bf16(const void* src, void* dst, int N, int K, void* stream) {
  return launch_pack_kstep_tiles((const bf16_t*)src, (bf16_t*)dst, N, K, ST);
}
int ptk_cast_f32_bf16(const float* in, void* out, int64_t n, void* stream) {
  return launch_cast_f32_bf16(in, (bf16_t*)out, n, ST);
}

int ptk_gemm_force_small_tiles(int mode) {
  if (mode != 0 && mode != 1 && mode != 2 && mode != 4 && mode != 8 && mode != 32 && mode != 512 && mode != 1024 &&
      mode != 4096)
    return set_error("gemm tile mode %d not in {0, 1, 2, 4, 8, 32, 512, 1024, 4096}", mode);
  force_small_tiles(mode);
  return 0;
}
int ptk_gemm_timer_enable(int on) {
  timer_enable(on);
  return 0;
}
int ptk_gemm_timer_read(int act_class, double* total_ms, int* count) { return timer_read(act_class, total_ms, count); }
int ptk_gemm_path_counts(int64_t* counts, int reset) { return path_counts(counts, reset); }
int ptk_gemm_ktiled_counts(int64_t* out2, int reset) { return ktiled_counts(out2, reset); }
int ptk_gemm_ktiled_pair(const ptk_gemm_desc* producer, const ptk_gemm_desc* consumer, int ncu, int64_t part_floats,
                         int train) {
  if (!producer || !consumer || ncu <= 0 || producer->batch > 1 || consumer->batch > 1) return 0;
  return !train && gemm_ktiled_pair(to_args(producer), producer->act, to_args(consumer), (long)part_floats,
                                    test_plan_env(ncu), a_ktiled_mode() != 0, true) ? 1 : 0;
}

int ptk_fill_normal_bf16(void* out, int64_t n, uint64_t seed, float std, float mean, void* stream) {
  return launch_fill_normal_bf16((bf16_t*)out, n, seed, std, mean, ST);
}

int ptk_flash_attn_fwd(const ptk_flash_desc* d, void* stream) {
  if (!d) return set_error("flash: null desc");
  FlashArgs a;
  a.Q = (const bf16_t*)d->Q; a.K = (const bf16_t*)d->K; a.V = (const bf16_t*)d->V; a.O = (bf16_t*)d->O;
  a.lse = d->lse; a.rows = d->rows; a.nkeys = d->nkeys; a.D = d->head_dim;
  a.ldq = d->ldq; a.ldk = d->ldk; a.ldo = d->ldo;
  a.zin = d->batch_inner > 0 ? d->batch_inner : 1; a.zdiv = d->zdiv > 0 ? d->zdiv : 1;
  a.sQ0 = d->sQ0; a.sQ1 = d->sQ1; a.sK0 = d->sK0; a.sK1 = d->sK1; a.sO0 = d->sO0; a.sO1 = d->sO1;
  a.qmap = to_map(d->qmap); a.omap = to_map(d->omap);
  a.qdiv = d->qdiv > 0 ? d->qdiv : 1; a.causal = d->causal; a.window = d->window;
  a.key_valid = d->key_valid; a.scale = d->scale;
  return launch_attn_fwd(a, d->batch > 0 ? d->batch : 1, ST);
}

static FlashBwdArgs to_bwd_args(const ptk_flash_bwd_desc* d) {
  FlashBwdArgs a;
  a.Q = (const bf16_t*)d->Q; a.K = (const bf16_t*)d->K; a.V = (const bf16_t*)d->V; a.O = (const bf16_t*)d->O;
  a.dO = (const bf16_t*)d->dO; a.lse = d->lse; a.delta = d->delta;
  a.dQ = (bf16_t*)d->dQ; a.dK = (bf16_t*)d->dK; a.dV = (bf16_t*)d->dV;
  a.rows = d->rows; a.nkeys = d->nkeys; a.D = d->head_dim;
  a.zin = d->batch_inner > 0 ? d->batch_inner : 1; a.zdiv = d->zdiv > 0 ? d->zdiv : 1;
  a.ldo = d->ldo; a.sO0 = d->sO0; a.sO1 = d->sO1; a.omap = to_map(d->omap);
  a.qdiv = d->qdiv > 0 ? d->qdiv : 1; a.causal = d->causal; a.window = d->window;
  a.key_valid = d->key_valid; a.scale = d->scale;
  a.dkv_part = (float*)d->workspace;
  a.dkv_part_bytes = d->workspace && d->workspace_bytes > 0 ? (size_t)d->workspace_bytes : 0;
  return a;
}

size_t ptk_flash_bwd_workspace_bytes(const ptk_flash_bwd_desc* d) {
  if (!d) return 0;
  return attn_bwd_workspace_bytes(to_bwd_args(d), d->batch > 0 ? d->batch : 1);
}

int ptk_flash_attn_bwd(const ptk_flash_bwd_desc* d, void* stream) {
  if (!d) return set_error("flash_bwd: null desc");
  return launch_attn_bwd(to_bwd_args(d), d->batch > 0 ? d->batch : 1, ST);
}

// ---------------------------------------------------------------- projector
int ptk_projector_fwd(const ptk_projector* p, int rows, const void* x, void* a, void* h, float* out,
                      ptk_rowmap out_map, int64_t ld_out, int round_bf16, void* stream) {
  const int Dv = p->vision_dim, I = p->inter_dim, Dl = p->llm_dim;
  TailScratchScope tail(p->tail_ws, ST);
  if (tail.status) return -1;
  StageScope stage("projector.fwd", ST);
  GemmArgs g1;
  g1.A = (const bf16_t*)x; g1.B = (const bf16_t*)p->w1; g1.C = h;
  g1.M = rows; g1.N = I; g1.K = Dv; g1.lda = Dv; g1.ldb = Dv; g1.ldc = I;
  g1.bias = p->b1; g1.aux = (bf16_t*)a; g1.ld_aux = I;
  if (launch_gemm(g1, ACT_GELU_ERF, OUT_BF16, 1, ST)) return -1;
  GemmArgs g2;
  g2.A = (const bf16_t*)h; g2.B = (const bf16_t*)p->w2; g2.C = out;
  g2.M = rows; g2.N = Dl; g2.K = I; g2.lda = I; g2.ldb = I; g2.ldc = ld_out;
  g2.bias = p->b2; g2.cmap = to_map(out_map);
  return launch_gemm(g2, ACT_NONE, round_bf16 ? OUT_F32_BFR : OUT_F32, 1, ST);
}

}  // extern "C"
static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
extern "C" {

size_t ptk_projector_workspace_bytes(const ptk_projector* p, int rows) {
  const size_t Dv = p->vision_dim, I = p->inter_dim, Dl = p->llm_dim, R = ((size_t)rows + 63) / 64 * 64;
  size_t s = 0;
  s += align256(Dl * R * 2);      // dy^T
  s += align256(I * R * 2);       // h^T, later dA^T
  s += align256(R * I * 2);       // dA
  s += align256(Dv * R * 2);      // x^T
  s += align256(64 * (I > Dl ? I : Dl) * 4);   // colsum partials
  return s;
}

}  // extern "C"

namespace ptk {
// stage 0: db2 = colsum(dy), dW2 = dy^T . h;  stage 1: dA = (dy . W2) * gelu'(a), db1 = colsum(dA), dW1 = dA^T . x
// (the projector backward in the order comm.cpp overlaps with the DDP exchange)
int projector_bwd_stage(const ptk_projector* p, int rows, const void* x, const void* a, const void* h, const void* dy,
                        float* dw1, float* db1, float* dw2, float* db2, void* ws, size_t ws_bytes, int stage,
                        hipStream_t st) {
  // weight grads contract over tokens: transposed operands are zero-padded to Rp = roundup(R, 64)
  const int Dv = p->vision_dim, I = p->inter_dim, Dl = p->llm_dim, R = rows, Rp = (rows + 63) / 64 * 64;
  if (ws_bytes < ptk_projector_workspace_bytes(p, rows)) return set_error("projector_bwd: workspace too small");
  char* w = (char*)ws;
  bf16_t* dyT = (bf16_t*)w; w += align256((size_t)Dl * Rp * 2);
  bf16_t* T = (bf16_t*)w; w += align256((size_t)I * Rp * 2);
  bf16_t* dA = (bf16_t*)w; w += align256((size_t)Rp * I * 2);
  bf16_t* xT = (bf16_t*)w; w += align256((size_t)Dv * Rp * 2);
  float* part = (float*)w;
  const long part_floats = 64L * (I > Dl ? I : Dl);   // the colsum partials of ptk_projector_workspace_bytes
  // the weight grads on the TN GEMM (gemm_tn.hip), which reads the token-major operands where they lie: K = Rp,
  // the rows R .. Rp - 1 past the operands' buffer ranges read as zero.  PTK_WGRAD_TN=0 (or operands the TN path
  // does not take): transposed copies for the NT GEMMs
  auto tn_wgrad = [&](const void* A, int lda, const void* B, int ldb, float* C, int M, int N) -> int {
    if (!wgrad_tn_enabled()) return 1;
    GemmArgs g;
    g.A = (const bf16_t*)A; g.B = (const bf16_t*)B; g.C = C; g.M = M; g.N = N; g.K = Rp;
    g.lda = lda; g.ldb = ldb; g.ldc = N;
    if (!tn_supported(g, OUT_F32, 1, lean_epilogue_enabled())) return 1;
    return gemm_tn(g, OUT_F32, 1, nullptr, st, R) ? -1 : 0;
  };
  if (stage == 0) {
    // db2 = colsum(dy); dW2 = dy^T . h  (contraction over tokens)
    if (launch_colsum_bf16((const bf16_t*)dy, R, Dl, db2, part, part_floats, st)) return -1;
    const int tn = tn_wgrad(dy, Dl, h, I, dw2, Dl, I);
    if (tn <= 0) return tn;
    if (launch_transpose((const bf16_t*)dy, Dl, 0, 0, 1, dyT, Rp, 0, 0, 1, R, Dl, Rp, st)) return -1;
    if (launch_transpose((const bf16_t*)h, I, 0, 0, 1, T, Rp, 0, 0, 1, R, I, Rp, st)) return -1;
    GemmArgs g;
    g.A = dyT; g.B = T; g.C = dw2; g.M = Dl; g.N = I; g.K = Rp; g.lda = Rp; g.ldb = Rp; g.ldc = I;
    return launch_gemm(g, ACT_NONE, OUT_F32, 1, st);
  }
  // dA = (dy . W2) * gelu'(a)
  GemmArgs g2;
  g2.A = (const bf16_t*)dy; g2.B = (const bf16_t*)p->w2t; g2.C = dA; g2.M = R; g2.N = I; g2.K = Dl;
  g2.lda = Dl; g2.ldb = Dl; g2.ldc = I; g2.aux_in = (const bf16_t*)a; g2.ld_aux_in = I;
  if (launch_gemm(g2, ACT_GELU_ERF_BWD, OUT_BF16, 1, st)) return -1;
  // db1 = colsum(dA); dW1 = dA^T . x
  if (launch_colsum_bf16(dA, R, I, db1, part, part_floats, st)) return -1;
  const int tn = tn_wgrad(dA, I, x, Dv, dw1, I, Dv);
  if (tn <= 0) return tn;
  if (launch_transpose(dA, I, 0, 0, 1, T, Rp, 0, 0, 1, R, I, Rp, st)) return -1;
  if (launch_transpose((const bf16_t*)x, Dv, 0, 0, 1, xT, Rp, 0, 0, 1, R, Dv, Rp, st)) return -1;
  GemmArgs g3;
  g3.A = T; g3.B = xT; g3.C = dw1; g3.M = I; g3.N = Dv; g3.K = Rp; g3.lda = Rp; g3.ldb = Rp; g3.ldc = Dv;
  return launch_gemm(g3, ACT_NONE, OUT_F32, 1, st);
}
}  // namespace ptk

extern "C" {

int ptk_projector_bwd(const ptk_projector* p, int rows, const void* x, const void* a, const void* h, const void* dy,
                      float* dw1, float* db1, float* dw2, float* db2, void* ws, size_t ws_bytes, void* stream) {
  TailScratchScope tail(p->tail_ws, ST);
  if (tail.status) return -1;
  StageScope stage("projector.bwd", ST);
  if (projector_bwd_stage(p, rows, x, a, h, dy, dw1, db1, dw2, db2, ws, ws_bytes, 0, ST)) return -1;
  return projector_bwd_stage(p, rows, x, a, h, dy, dw1, db1, dw2, db2, ws, ws_bytes, 1, ST);
}

// Stage 2's trainable projector (bf16 parameters and .grad, Stage2/trainer.py:214-223,336-337 under
// --mixed_precision bf16): the four grads ACCUMULATED as autograd does into a bf16 .grad, bf16(grad + bf16(G)).
// Workspace: dA | ta | tb (the NT path's transposed operands) | the column sums' partials.
size_t ptk_projector_bwd_bf16_workspace_bytes(const ptk_projector* p, int rows) {
  if (!p || rows <= 0) return 0;
  const size_t Dv = p->vision_dim, I = p->inter_dim, Dl = p->llm_dim, R = ((size_t)rows + 63) / 64 * 64;
  size_t s = 0;
  s += align256(R * I * 2);                       // dA
  s += align256((I > Dl ? I : Dl) * R * 2);       // ta: dy^T, then dA^T
  s += align256((I > Dv ? I : Dv) * R * 2);       // tb: h^T, then x^T
  s += align256(64 * (I > Dl ? I : Dl) * 4);      // colsum partials
  return s;
}

}  // extern "C"

// ptk_projector_bwd_bf16 and ptk_projector_input_grad.  grads: the four parameter grads are accumulated (the
// trained projector); dx_vis != null: the input grad bf16(dA W1) as well, W1^T transposed into w1t first
static int projector_bwd_bf16_run(const ptk_projector* p, int rows, const void* x, const void* a, const void* h,
                                  const void* dy, void* dw1, void* db1, void* dw2, void* db2, void* dx_vis,
                                  void* ws, bf16_t* w1t, void* stream) {
  const bool grads = dw1 != nullptr;
  const int Dv = p->vision_dim, I = p->inter_dim, Dl = p->llm_dim, R = rows;
  const size_t Rp = ((size_t)R + 63) / 64 * 64;
  char* w = (char*)ws;
  bf16_t* dA = (bf16_t*)w; w += align256(Rp * I * 2);
  bf16_t* ta = (bf16_t*)w; w += align256((size_t)(I > Dl ? I : Dl) * Rp * 2);
  bf16_t* tb = (bf16_t*)w; w += align256((size_t)(I > Dv ? I : Dv) * Rp * 2);
  float* cpart = (float*)w;
  const long cpart_floats = 64L * (I > Dl ? I : Dl);
  // the weight grads' fp32 scratch (stream-K slabs of the TN GEMM, K slices of the NT one): the projector's tail
  // scratch, which this call's GEMMs use one after the other on the stream
  float* part = (float*)p->tail_ws;
  const int64_t part_floats = part ? (int64_t)(p8_tail_scratch_bytes() / sizeof(float)) : 0;
  // rows a multiple of 64 (B x 576 patches in a real run): the TN GEMM on the token-major operands in place;
  // a ragged row count: the transposed, zero-padded copies for the NT GEMMs
  const int mode = R % 64 == 0 ? 0 : 1;
  StageScope stage("projector.bwd", ST);
  if (grads) {
    // db2 += colsum(dy); dW2 += dy^T . h
    if (launch_colsum_bf16_acc((const bf16_t*)dy, R, Dl, (bf16_t*)db2, cpart, cpart_floats, ST)) return -1;
    if (ptk_weight_grad_bf16(dy, Dl, 0, 0, 0, Dl, h, I, 0, 0, 0, I, R, dw2, ta, tb, part, part_floats, mode, stream))
      return -1;
  }
  // dA = bf16((dy . W2) * gelu'(a))
  GemmArgs g2;
  g2.A = (const bf16_t*)dy; g2.B = (const bf16_t*)p->w2t; g2.C = dA; g2.M = R; g2.N = I; g2.K = Dl;
  g2.lda = Dl; g2.ldb = Dl; g2.ldc = I; g2.aux_in = (const bf16_t*)a; g2.ld_aux_in = I;
  {   // (the tail scratch is lent to this GEMM alone: the weight grads hold it as `part`)
    TailScratchScope tail(p->tail_ws, ST);
    if (tail.status || launch_gemm(g2, ACT_GELU_ERF_BWD, OUT_BF16, 1, ST)) return -1;
  }
  if (grads) {
    // db1 += colsum(dA); dW1 += dA^T . x
    if (launch_colsum_bf16_acc(dA, R, I, (bf16_t*)db1, cpart, cpart_floats, ST)) return -1;
    if (ptk_weight_grad_bf16(dA, I, 0, 0, 0, I, x, Dv, 0, 0, 0, Dv, R, dw1, ta, tb, part, part_floats, mode, stream))
      return -1;
  }
  if (!dx_vis) return 0;
  // dx_vis = bf16(dA . W1): W1 [I, Dv] -> W1^T [Dv, I], the K-contiguous B of the NT GEMM
  if (launch_transpose((const bf16_t*)p->w1, Dv, 0, 0, 1, w1t, I, 0, 0, 1, I, Dv, I, ST)) return -1;
  GemmArgs g3;
  g3.A = dA; g3.B = w1t; g3.C = dx_vis; g3.M = R; g3.N = Dv; g3.K = I; g3.lda = I; g3.ldb = I; g3.ldc = Dv;
  TailScratchScope tail(p->tail_ws, ST);
  if (tail.status) return -1;
  return launch_gemm(g3, ACT_NONE, OUT_BF16, 1, ST);
}

extern "C" {

int ptk_projector_bwd_bf16(const ptk_projector* p, int rows, const void* x, const void* a, const void* h,
                           const void* dy, void* dw1, void* db1, void* dw2, void* db2, void* ws, size_t ws_bytes,
                           void* stream) {
  if (!p || !x || !a || !h || !dy || !dw1 || !db1 || !dw2 || !db2 || !ws)
    return set_error("projector_bwd_bf16: null argument");
  if (!p->w2t) return set_error("projector_bwd_bf16: the projector has no W2^T");
  const int Dv = p->vision_dim, I = p->inter_dim, Dl = p->llm_dim, R = rows;
  if (R <= 0 || Dv <= 0 || I <= 0 || Dl <= 0) return set_error("projector_bwd_bf16: rows %d dims %d %d %d", R, Dv, I, Dl);
  if (Dv % 8 || I % 8 || Dl % 8) return set_error("projector_bwd_bf16: dims %d %d %d must be multiples of 8", Dv, I, Dl);
  if (ws_bytes < ptk_projector_bwd_bf16_workspace_bytes(p, rows)) return set_error("projector_bwd_bf16: workspace too small");
  if ((uintptr_t)ws & 15) return set_error("projector_bwd_bf16: workspace must be 16-byte aligned");
  return projector_bwd_bf16_run(p, rows, x, a, h, dy, dw1, db1, dw2, db2, nullptr, ws, nullptr, stream);
}

// Workspace: ptk_projector_bwd_bf16's, then W1^T
size_t ptk_projector_input_grad_workspace_bytes(const ptk_projector* p, int rows) {
  if (!p || rows <= 0) return 0;
  return ptk_projector_bwd_bf16_workspace_bytes(p, rows) + align256((size_t)p->vision_dim * p->inter_dim * 2);
}

int ptk_projector_input_grad(const ptk_projector* p, int rows, const void* x, const void* a, const void* h,
                             const void* dy, void* dw1, void* db1, void* dw2, void* db2, void* dx_vis, void* ws,
                             size_t ws_bytes, void* stream) {
  if (!p || !a || !dy || !dx_vis || !ws) return set_error("projector_input_grad: null argument");
  const bool grads = dw1 || db1 || dw2 || db2;
  if (grads && (!dw1 || !db1 || !dw2 || !db2 || !x || !h))
    return set_error("projector_input_grad: the four parameter grads (with x and h) go together, or all NULL");
  if (!p->w1 || !p->w2t) return set_error("projector_input_grad: the projector has no W1 / W2^T");
  const int Dv = p->vision_dim, I = p->inter_dim, Dl = p->llm_dim, R = rows;
  if (R <= 0 || Dv <= 0 || I <= 0 || Dl <= 0) return set_error("projector_input_grad: rows %d dims %d %d %d", R, Dv, I, Dl);
  if (Dv % 64 || I % 64 || Dl % 64)
    return set_error("projector_input_grad: dims %d %d %d must be multiples of 64", Dv, I, Dl);
  if (ws_bytes < ptk_projector_input_grad_workspace_bytes(p, rows)) return set_error("projector_input_grad: workspace too small");
  if ((uintptr_t)ws & 15) return set_error("projector_input_grad: workspace must be 16-byte aligned");
  bf16_t* w1t = (bf16_t*)((char*)ws + ptk_projector_bwd_bf16_workspace_bytes(p, rows));
  return projector_bwd_bf16_run(p, rows, x, a, h, dy, dw1, db1, dw2, db2, dx_vis, ws, w1t, stream);
}

int ptk_gather_vision_grad(const float* dx_llm, int batch, int num_patches, int seq_pad, int llm_dim, void* dy,
                           void* stream) {
  return launch_gather_dy(dx_llm, batch, num_patches, seq_pad, llm_dim, (bf16_t*)dy, ST);
}

// ---------------------------------------------------------------- optimizer
int ptk_clip_adamw(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float grad_scale,
                   float max_norm, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                   float* partial, float* norm_out, void* stream) {
  if (step < 1) return set_error("clip_adamw: step must be >= 1");
  if ((uintptr_t)grads & 15) return set_error("clip_adamw: grads must be 16-byte aligned");
  const int nparts = 1024;
  if (launch_sumsq_partial(grads, n, partial, nparts, ST)) return -1;
  return launch_clip_adamw(params, grads, exp_avg, exp_avg_sq, n, partial, nparts, grad_scale, max_norm, lr, beta1,
                           beta2, eps, weight_decay, step, norm_out, ST);
}

}  // extern "C"
