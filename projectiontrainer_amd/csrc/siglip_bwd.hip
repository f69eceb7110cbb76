// Side kernels of the SigLIP vision tower's backward (Stage 2 with the tower trained; models.cpp ptk_siglip_bwd).
// All HBM-bound: 16-byte accesses, fp32 arithmetic, no floating-point atomics (every sum has a fixed order, so a
// repeated call from the same state is bit-identical).
//
//   layernorm_bwd   d/dx of nn.LayerNorm over bf16 rows (modeling_siglip.py:329,331,567) with the residual
//                   stream's grad added in, plus fp32 per-workgroup partials of dw = colsum(dy xhat), db = colsum(dy)
//                   (finished by train.hip's fixed-order fold and bf16 accumulate, launch_rms_wgrad_finish)
//   gelu_tanh_bwd   dpre = bf16(dg * gelu_tanh'(pre)), the derivative of the fc1 epilogue's ACT_GELU_TANH
//   pos_grad        dpos[n] += bf16(sum_b dh0[b N + n]), batches in index order
//   heads_split / heads_merge
//                   token-major [B N][ld] column blocks <-> head-major [B H][N][hd], the dense layout
//                   ptk_flash_attn_bwd takes for Q, K, V, dO and returns dQ, dK, dV in
#include "common.h"
#include "ptk_internal.h"

namespace ptk {

#define RET_OK(name) return hipGetLastError() == hipSuccess ? 0 : set_error(name " launch failed")

namespace {

PTK_DEV void ld8(const bf16_t* p, float* v) {
  const u16x8_t u = *reinterpret_cast<const u16x8_t*>(p);
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = bf2f(u[e]);
}
PTK_DEV void st8(bf16_t* p, const float* v) {
  u16x8_t u;
#pragma unroll
  for (int e = 0; e < 8; ++e) u[e] = f2bf(v[e]);
  *reinterpret_cast<u16x8_t*>(p) = u;
}
PTK_DEV void ld8f(const float* p, float* v) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
PTK_DEV void st8f(float* p, const float* v) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}

// ---------------------------------------------------------------- LayerNorm backward
// y = xhat w + b, xhat = (x - mean) rstd (statistics recomputed from x as the forward computes them, norm.hip):
//   g = dy w;  dx = rstd (g - mean(g) - xhat mean(g xhat));  dw = sum_r dy xhat;  db = sum_r dy
// One wave per row, the row in registers (8 columns per lane and 512-column group, cols <= 512 NV); a block of 4
// waves walks LNB_ROWS rows (wave v: rows r0 + v, r0 + v + 4, ...) keeping its dw / db sums in registers, the four
// waves' sums are added in wave order through LDS and stored as the block's partial row.
constexpr int LNB_ROWS = 32;
constexpr int LNB_MAXV = 4;   // cols <= 2048

template <int NV>
__global__ void __launch_bounds__(256) layernorm_bwd_kernel(const bf16_t* __restrict__ x, const float* __restrict__ w,
                                                            const bf16_t* __restrict__ dy, const bf16_t* dacc,
                                                            bf16_t* dx, int rows, int cols, float eps,
                                                            float* __restrict__ part_w, float* __restrict__ part_b) {
  __shared__ float red[3][2][NV][64][8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r0 = blockIdx.x * LNB_ROWS, r1 = min(rows, r0 + LNB_ROWS);
  float wv[NV][8], sw[NV][8], sb[NV][8];
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int c = lane * 8 + v * 512;
#pragma unroll
    for (int e = 0; e < 8; ++e) wv[v][e] = sw[v][e] = sb[v][e] = 0.f;
    if (c < cols) ld8f(w + c, wv[v]);
  }
  const float inv = 1.f / (float)cols;
  for (int r = r0 + wave; r < r1; r += 4) {
    float xv[NV][8], gv[NV][8];
    float s = 0.f;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int c = lane * 8 + v * 512;
#pragma unroll
      for (int e = 0; e < 8; ++e) xv[v][e] = gv[v][e] = 0.f;
      if (c < cols) {
        ld8(x + (long)r * cols + c, xv[v]);
        ld8(dy + (long)r * cols + c, gv[v]);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) s += xv[v][e];
    }
    const float mean = warp_sum(s) / cols;
    float q = 0.f;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const bool in = lane * 8 + v * 512 < cols;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        xv[v][e] = in ? xv[v][e] - mean : 0.f;
        q += xv[v][e] * xv[v][e];
      }
    }
    const float rstd = rsqrtf(warp_sum(q) / cols + eps);
    float sg = 0.f, sgx = 0.f;
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float xh = xv[v][e] * rstd, d = gv[v][e];
        xv[v][e] = xh;
        sw[v][e] += d * xh;
        sb[v][e] += d;
        const float g = d * wv[v][e];
        gv[v][e] = g;
        sg += g;
        sgx += g * xh;
      }
    const float mg = warp_sum(sg) * inv, mgx = warp_sum(sgx) * inv;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int c = lane * 8 + v * 512;
      if (c < cols) {
        float o[8], a[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = rstd * (gv[v][e] - mg - xv[v][e] * mgx);
        if (dacc) {   // (may alias dx: a lane reads its own 8 columns before it stores them)
          ld8(dacc + (long)r * cols + c, a);
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] += a[e];
        }
        st8(dx + (long)r * cols + c, o);
      }
    }
  }
  if (!part_w) return;
  if (wave > 0) {
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        red[wave - 1][0][v][lane][e] = sw[v][e];
        red[wave - 1][1][v][lane][e] = sb[v][e];
      }
  }
  __syncthreads();
  if (wave > 0) return;
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        sw[v][e] += red[k][0][v][lane][e];
        sb[v][e] += red[k][1][v][lane][e];
      }
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int c = lane * 8 + v * 512;
    if (c < cols) {
      st8f(part_w + (long)blockIdx.x * cols + c, sw[v]);
      st8f(part_b + (long)blockIdx.x * cols + c, sb[v]);
    }
  }
}

// ---------------------------------------------------------------- GELU-tanh backward
__global__ void __launch_bounds__(256) gelu_tanh_bwd_kernel(const bf16_t* dg, const bf16_t* __restrict__ pre,
                                                            bf16_t* dpre, long n8) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  float d[8], p[8];
  ld8(dg + i * 8, d);
  ld8(pre + i * 8, p);
#pragma unroll
  for (int e = 0; e < 8; ++e) d[e] *= gelu_tanh_grad(p[e]);
  st8(dpre + i * 8, d);
}

// ---------------------------------------------------------------- position-embedding grad
__global__ void __launch_bounds__(256) pos_grad_kernel(const bf16_t* __restrict__ dh0, int B, long nd8,
                                                       bf16_t* __restrict__ dpos) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;   // 8-column unit of the [N][D] table
  if (i >= nd8) return;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, v[8];
  for (int b = 0; b < B; ++b) {
    ld8(dh0 + ((long)b * nd8 + i) * 8, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] += v[e];
  }
  ld8(dpos + i * 8, v);
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] += bfround(s[e]);
  st8(dpos + i * 8, v);
}

// ---------------------------------------------------------------- token-major <-> head-major
// unit u (16 bytes) of the head-major side [B][H][N][hd]: (b, h, n, j) <-> tok[(b N + n) ld + h hd + 8 j]
template <bool SPLIT>
__global__ void __launch_bounds__(256) heads_kernel(bf16_t* tok, long ld, bf16_t* heads, int N, int H, int hd8,
                                                    long units) {
  const long u = (long)blockIdx.x * 256 + threadIdx.x;
  if (u >= units) return;
  long t = u;
  const int j = (int)(t % hd8); t /= hd8;
  const int n = (int)(t % N); t /= N;
  const int h = (int)(t % H);
  const long b = t / H;
  bf16_t* tp = tok + (b * N + n) * ld + ((long)h * hd8 + j) * 8;
  bf16_t* hp = heads + u * 8;
  if (SPLIT) *reinterpret_cast<uint4*>(hp) = *reinterpret_cast<const uint4*>(tp);
  else *reinterpret_cast<uint4*>(tp) = *reinterpret_cast<const uint4*>(hp);
}

}  // namespace

int layernorm_bwd_blocks(int rows) { return (rows + LNB_ROWS - 1) / LNB_ROWS; }
long layernorm_bwd_partial_floats(int rows, int cols) {
  return 2L * rms_wgrad_finish_floats(layernorm_bwd_blocks(rows), cols);
}

int launch_layernorm_bwd_bf16(const bf16_t* x, const float* w, const bf16_t* dy, const bf16_t* dacc, bf16_t* dx,
                              int rows, int cols, float eps, bf16_t* dw, bf16_t* db, float* partial,
                              long part_floats, hipStream_t st) {
  if (rows <= 0) return 0;
  if (cols <= 0 || cols % 8 || cols > 512 * LNB_MAXV)
    return set_error("layernorm_bwd: cols %d (a multiple of 8, <= %d)", cols, 512 * LNB_MAXV);
  if (!x || !w || !dy || !dx) return set_error("layernorm_bwd: null argument");
  if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)dy | (uintptr_t)dacc | (uintptr_t)dx | (uintptr_t)partial) & 15)
    return set_error("layernorm_bwd: operands must be 16-byte aligned");
  if ((dw == nullptr) != (db == nullptr)) return set_error("layernorm_bwd: dw and db go together");
  const int nblk = layernorm_bwd_blocks(rows);
  float *pw = nullptr, *pb = nullptr;
  if (dw) {
    if (!partial || part_floats < layernorm_bwd_partial_floats(rows, cols))
      return set_error("layernorm_bwd: partial scratch of %ld floats, %ld needed", part_floats,
                       layernorm_bwd_partial_floats(rows, cols));
    pw = partial;
    pb = partial + rms_wgrad_finish_floats(nblk, cols);
  }
  const dim3 g((unsigned)nblk);
  switch ((cols + 511) / 512) {
    case 1: hipLaunchKernelGGL(layernorm_bwd_kernel<1>, g, dim3(256), 0, st, x, w, dy, dacc, dx, rows, cols, eps, pw, pb); break;
    case 2: hipLaunchKernelGGL(layernorm_bwd_kernel<2>, g, dim3(256), 0, st, x, w, dy, dacc, dx, rows, cols, eps, pw, pb); break;
    case 3: hipLaunchKernelGGL(layernorm_bwd_kernel<3>, g, dim3(256), 0, st, x, w, dy, dacc, dx, rows, cols, eps, pw, pb); break;
    default: hipLaunchKernelGGL(layernorm_bwd_kernel<4>, g, dim3(256), 0, st, x, w, dy, dacc, dx, rows, cols, eps, pw, pb); break;
  }
  if (hipGetLastError() != hipSuccess) return set_error("layernorm_bwd launch failed");
  if (!dw) return 0;
  if (launch_rms_wgrad_finish(pw, nblk, cols, dw, st)) return -1;
  return launch_rms_wgrad_finish(pb, nblk, cols, db, st);
}

int launch_gelu_tanh_bwd_bf16(const bf16_t* dg, const bf16_t* pre, bf16_t* dpre, long rows, int cols, hipStream_t st) {
  if (rows <= 0 || cols <= 0) return 0;
  if (cols % 8) return set_error("gelu_tanh_bwd: cols %d must be a multiple of 8", cols);
  if (!dg || !pre || !dpre || (((uintptr_t)dg | (uintptr_t)pre | (uintptr_t)dpre) & 15))
    return set_error("gelu_tanh_bwd: operands must be non-null and 16-byte aligned");
  const long n8 = rows * cols / 8;
  hipLaunchKernelGGL(gelu_tanh_bwd_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, st, dg, pre, dpre, n8);
  RET_OK("gelu_tanh_bwd");
}

int launch_pos_grad_bf16(const bf16_t* dh0, int B, int N, int D, bf16_t* dpos, hipStream_t st) {
  if (B <= 0 || N <= 0 || D <= 0) return 0;
  if (D % 8) return set_error("pos_grad: hidden %d must be a multiple of 8", D);
  if (!dh0 || !dpos || (((uintptr_t)dh0 | (uintptr_t)dpos) & 15))
    return set_error("pos_grad: operands must be non-null and 16-byte aligned");
  const long nd8 = (long)N * D / 8;
  hipLaunchKernelGGL(pos_grad_kernel, dim3((unsigned)((nd8 + 255) / 256)), dim3(256), 0, st, dh0, B, nd8, dpos);
  RET_OK("pos_grad");
}

static int heads_launch(bool split, bf16_t* tok, long ld, bf16_t* heads, int B, int N, int H, int hd, hipStream_t st) {
  if (B <= 0 || N <= 0 || H <= 0) return 0;
  if (hd % 8 || ld % 8 || ld < (long)H * hd || (((uintptr_t)tok | (uintptr_t)heads) & 15))
    return set_error("heads_split/merge: head_dim %d, row stride %ld", hd, ld);
  const long units = (long)B * H * N * (hd / 8);
  const dim3 g((unsigned)((units + 255) / 256));
  if (split) hipLaunchKernelGGL(heads_kernel<true>, g, dim3(256), 0, st, tok, ld, heads, N, H, hd / 8, units);
  else hipLaunchKernelGGL(heads_kernel<false>, g, dim3(256), 0, st, tok, ld, heads, N, H, hd / 8, units);
  RET_OK("heads_split/merge");
}
int launch_heads_split(const bf16_t* tok, long ld, bf16_t* heads, int B, int N, int H, int hd, hipStream_t st) {
  return heads_launch(true, const_cast<bf16_t*>(tok), ld, heads, B, N, H, hd, st);
}
int launch_heads_merge(const bf16_t* heads, bf16_t* tok, long ld, int B, int N, int H, int hd, hipStream_t st) {
  return heads_launch(false, tok, ld, const_cast<bf16_t*>(heads), B, N, H, hd, st);
}

}  // namespace ptk
