// Linear-probe head (trainers/linear_prob.py:85-95 + F.cross_entropy, :151-184): a dense e x e layer plus bias on the
// UN-normalised image features, cosine-free logits against fixed normalised text features, and the gradient of the layer
// itself.  Four launches for a training call, two for eval; every GEMM-shaped part on the fp32 matrix pipe
// (v_mfma_f32_32x32x2_f32: exact fp32 products, one rounding per fma, fixed k order) and every sum in a fixed order, so the
// bits repeat from call to call and under graph replay.
//   lp_z:      z = img_f . w^T + bias                         tile (32 images x 32 outputs), split-k over the waves
//   lp_logits: logits = scale * z . text_f_n^T                tile (32 images x 32 classes), split-k over the waves; per
//              (image, class tile) row max and sum of exp(logit - max) into the workspace
//   lp_dz:     lse from the partials (fixed tile order); dz = G . text_f_n with G = scale (softmax - onehot) / B formed on
//              the fly (split-k over the classes); block (0, 0) also writes the batch-mean loss
//   lp_gw:     g_w = dz^T . img_f (K = B), g_bias = sum_b dz  (the blocks of input tile 0)
// rpo_lp_head_fwd_bwd_grouped runs S such heads (the members of a linear-probe sweep: one layer each, shared features,
// text features and labels) in the same four launches with the group as blockIdx.z, through the same tile functions.
#include "common.h"

namespace {

constexpr int LP_WAVES = 8;                    // split-k waves of the three launches with a long k
constexpr int LP_MAX_B = 128, LP_MAX_E = 1024, LP_MAX_C = 32768, LP_MAX_S = 1024;

// acc[r] of v_mfma_f32_32x32x2_f32 is D[(r & 3) + 8 (r >> 2) + 4 half][l31]; operands: lane (l31, half) gives A[l31][k0 + half]
// and B[k0 + half][l31] (rpo_probe_mfma pins both maps; misc.hip's head kernels use the same)
__device__ __forceinline__ int lp_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

__device__ __forceinline__ f32x16_t lp_zero() {
  f32x16_t d;
#pragma unroll
  for (int r = 0; r < 16; ++r) d[r] = 0.f;
  return d;
}

// D[m][n] += sum_{k in [k0, k1)} A[m][k] Bt[n][k] for both operands row-major with k contiguous (the "NT" form of z and of
// the logits).  (k1 - k0) % 8 == 0.  Rows past the matrix are clamped for the loads; their results are never stored.
__device__ __forceinline__ f32x16_t lp_tile_nt(const float* __restrict__ a, const float* __restrict__ bt, int k0, int k1,
                                               f32x16_t d, int half) {
  const float* pa = a + 4 * half;
  const float* pb = bt + 4 * half;
  for (int k = k0; k < k1; k += 8) {                              // lane half h holds k .. k+7's elements 4h .. 4h+3
    const float4 av = *reinterpret_cast<const float4*>(pa + k);
    const float4 bv = *reinterpret_cast<const float4*>(pb + k);
    d = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, d, 0, 0, 0);
    d = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, d, 0, 0, 0);
    d = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, d, 0, 0, 0);
    d = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, d, 0, 0, 0);
  }
  return d;
}

// The k range of wave w when [0, K) is split over LP_WAVES waves in chunks of a multiple of `q` elements.
__device__ __forceinline__ void lp_split(int K, int q, int w, int& k0, int& k1) {
  const int per = ((K + LP_WAVES - 1) / LP_WAVES + q - 1) / q * q;
  k0 = min(K, w * per);
  k1 = min(K, k0 + per);
}

// Sum of the LP_WAVES partial tiles in wave order (fixed): every wave parks its 16 accumulators in LDS, wave 0 adds them.
__device__ __forceinline__ f32x16_t lp_reduce(f32x16_t d, float* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < 16; ++r) red[(w * 16 + r) * 64 + lane] = d[r];
  __syncthreads();
  f32x16_t s = lp_zero();
  if (w == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float v = red[r * 64 + lane];
      for (int j = 1; j < LP_WAVES; ++j) v += red[(j * 16 + r) * 64 + lane];
      s[r] = v;
    }
  }
  return s;
}

// The four tiles as device functions: the ungrouped kernels call them on the caller's arrays, the grouped ones on group
// blockIdx.z's slices (same instructions per tile either way, so a group has the bits of the ungrouped call).
__device__ __forceinline__ void lp_z_tile(const float* __restrict__ x, const float* __restrict__ w,
                                          const float* __restrict__ bias, float* z, int B, int e) {
  __shared__ float red[LP_WAVES * 16 * 64];
  const int lane = threadIdx.x & 63, l31 = lane & 31, half = lane >> 5, wv = threadIdx.x >> 6;
  const int j0 = blockIdx.x * 32, b0 = blockIdx.y * 32;
  int k0, k1;
  lp_split(e, 8, wv, k0, k1);
  const f32x16_t d = lp_tile_nt(x + (int64_t)min(b0 + l31, B - 1) * e, w + (int64_t)(j0 + l31) * e, k0, k1, lp_zero(), half);
  const f32x16_t s = lp_reduce(d, red);
  if (wv != 0) return;
  const float bj = bias[j0 + l31];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int b = b0 + lp_row(r, half);
    if (b < B) z[(int64_t)b * e + j0 + l31] = s[r] + bj;
  }
}

// logits tile + per-row partial softmax statistics of its 32 classes: pmax / psum [C tiles][B]
__device__ __forceinline__ void lp_logits_tile(const float* __restrict__ z, const float* __restrict__ t, float* logits,
                                               float* pmax, float* psum, float scale, int B, int C, int e) {
  __shared__ float red[LP_WAVES * 16 * 64];
  const int lane = threadIdx.x & 63, l31 = lane & 31, half = lane >> 5, wv = threadIdx.x >> 6;
  const int c0 = blockIdx.x * 32, b0 = blockIdx.y * 32;
  const int c = c0 + l31;
  int k0, k1;
  lp_split(e, 8, wv, k0, k1);
  const f32x16_t d = lp_tile_nt(z + (int64_t)min(b0 + l31, B - 1) * e, t + (int64_t)min(c, C - 1) * e, k0, k1, lp_zero(),
                                half);
  const f32x16_t s = lp_reduce(d, red);
  if (wv != 0) return;
  const bool cok = c < C;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int b = b0 + lp_row(r, half);
    const float v = s[r] * scale;
    if (cok && b < B) logits[(int64_t)b * C + c] = v;
    // row statistics over the 32 classes of the tile: butterfly inside the lane half (fixed order)
    float m = cok ? v : -INFINITY;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    float se = cok ? expf(v - m) : 0.f;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) se += __shfl_xor(se, o, 64);
    if (l31 == 0 && b < B) {
      pmax[(int64_t)blockIdx.x * B + b] = m;
      psum[(int64_t)blockIdx.x * B + b] = se;
    }
  }
}

// log-sum-exp of row b from the per-tile partials, tiles in order
__device__ __forceinline__ void lp_row_stats(const float* __restrict__ pmax, const float* __restrict__ psum, int b, int B,
                                             int ct, float& m, float& s) {
  m = -INFINITY;
  for (int i = 0; i < ct; ++i) m = fmaxf(m, pmax[(int64_t)i * B + b]);
  s = 0.f;
  for (int i = 0; i < ct; ++i) s += psum[(int64_t)i * B + b] * expf(pmax[(int64_t)i * B + b] - m);
}

// dz[b][j] = sum_c G[b][c] t[c][j], G[b][c] = gmul (exp(logit - m_b) / s_b - [c == label_b]) (+ NaN for a bad label)
__device__ __forceinline__ void lp_dz_tile(const float* __restrict__ logits, const float* __restrict__ t,
                                           const float* __restrict__ pmax, const float* __restrict__ psum,
                                           const int64_t* __restrict__ label, float* dz, float* loss, float gmul, int B, int C,
                                           int e) {
  __shared__ float red[LP_WAVES * 16 * 64];
  __shared__ float s_m[32], s_inv[32], s_poison[32];
  __shared__ int s_lb[32];
  __shared__ float s_loss[LP_MAX_B];
  const int lane = threadIdx.x & 63, l31 = lane & 31, half = lane >> 5, wv = threadIdx.x >> 6;
  const int j0 = blockIdx.x * 32, b0 = blockIdx.y * 32;
  const int ct = (C + 31) / 32;
  if (threadIdx.x < 32) {
    const int b = min(b0 + threadIdx.x, B - 1);
    float m, s;
    lp_row_stats(pmax, psum, b, B, ct, m, s);
    const int64_t lb64 = label[b];
    const bool ok = lb64 >= 0 && lb64 < C;
    s_m[threadIdx.x] = m;
    s_inv[threadIdx.x] = 1.0f / s;
    s_lb[threadIdx.x] = ok ? (int)lb64 : -1;
    s_poison[threadIdx.x] = ok ? 0.0f : __builtin_nanf("");
  }
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < B) {     // the batch-mean loss: one block owns it
    const int b = threadIdx.x;
    float m, s;
    lp_row_stats(pmax, psum, b, B, ct, m, s);
    const int64_t lb64 = label[b];
    const bool ok = lb64 >= 0 && lb64 < C;                         // F.cross_entropy raises; a kernel cannot: NaN
    s_loss[b] = ok ? (m + logf(s)) - logits[(int64_t)b * C + lb64] : __builtin_nanf("");
  }
  __syncthreads();
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
    float acc = 0.f;
    for (int b = 0; b < B; ++b) acc += s_loss[b];
    loss[0] = acc / (float)B;
  }
  // A operand: G[b0 + l31][k], B operand: t[k][j0 + l31]; k = class, split over the waves in even chunks
  int k0, k1;
  lp_split(C, 2, wv, k0, k1);
  const bool bok = b0 + l31 < B;
  const int bl = min(b0 + l31, B - 1);
  const float* lrow = logits + (int64_t)bl * C;
  const float m = s_m[l31], inv = s_inv[l31], poison = s_poison[l31];
  const int lb = s_lb[l31];
  f32x16_t d = lp_zero();
  for (int k = k0; k < k1; k += 2) {
    const int kc = k + half;
    const bool kok = kc < k1;
    const int kk = kok ? kc : k0;                                  // (k0 < k1 here: a valid class to read)
    const float g = (bok && kok) ? (expf(lrow[kk] - m) * inv - (kk == lb ? 1.0f : 0.0f)) * gmul + poison : 0.f;
    const float tv = kok ? t[(int64_t)kk * e + j0 + l31] : 0.f;
    d = __builtin_amdgcn_mfma_f32_32x32x2f32(g, tv, d, 0, 0, 0);
  }
  const f32x16_t s = lp_reduce(d, red);
  if (wv != 0) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int b = b0 + lp_row(r, half);
    if (b < B) dz[(int64_t)b * e + j0 + l31] = s[r];
  }
}

// g_w[j][i] = sum_b dz[b][j] x[b][i]  (one wave per 32 x 32 tile, k = b in order); g_bias[j] = sum_b dz[b][j] (input tile 0)
__device__ __forceinline__ void lp_gw_tile(const float* __restrict__ dz, const float* __restrict__ x, float* g_w,
                                           float* g_bias, int B, int e) {
  const int lane = threadIdx.x, l31 = lane & 31, half = lane >> 5;
  const int j0 = blockIdx.x * 32, i0 = blockIdx.y * 32;
  f32x16_t d = lp_zero();
  for (int k = 0; k < B; k += 2) {
    const int kb = k + half;
    const bool ok = kb < B;
    const int kr = ok ? kb : 0;
    const float a = ok ? dz[(int64_t)kr * e + j0 + l31] : 0.f;
    const float b = ok ? x[(int64_t)kr * e + i0 + l31] : 0.f;
    d = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, d, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) g_w[(int64_t)(j0 + lp_row(r, half)) * e + i0 + l31] = d[r];
  if (blockIdx.y == 0 && half == 0) {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += dz[(int64_t)b * e + j0 + l31];
    g_bias[j0 + l31] = s;
  }
}

__global__ __launch_bounds__(64 * LP_WAVES) void lp_z_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                             const float* __restrict__ bias, float* z, int B, int e) {
  lp_z_tile(x, w, bias, z, B, e);
}

__global__ __launch_bounds__(64 * LP_WAVES) void lp_logits_kernel(const float* __restrict__ z, const float* __restrict__ t,
                                                                  float* logits, float* pmax, float* psum, float scale,
                                                                  int B, int C, int e) {
  lp_logits_tile(z, t, logits, pmax, psum, scale, B, C, e);
}

__global__ __launch_bounds__(64 * LP_WAVES) void lp_dz_kernel(const float* __restrict__ logits, const float* __restrict__ t,
                                                              const float* __restrict__ pmax, const float* __restrict__ psum,
                                                              const int64_t* __restrict__ label, float* dz, float* loss,
                                                              float gmul, int B, int C, int e) {
  lp_dz_tile(logits, t, pmax, psum, label, dz, loss, gmul, B, C, e);
}

__global__ __launch_bounds__(64) void lp_gw_kernel(const float* __restrict__ dz, const float* __restrict__ x, float* g_w,
                                                   float* g_bias, int B, int e) {
  lp_gw_tile(dz, x, g_w, g_bias, B, e);
}

// ---- S heads in the launches of one: group s = blockIdx.z.  Its layer is row s of `params` = [W_s (e x e) | b_s (e)] (row
// stride `ps` floats, the gradient in the same layout), its z / logits / loss are slice s of [S, B, e] / [S, B, C] / [S],
// its workspace is slice s of S slices of `wsf` floats = [dz (B e) | pmax (ct B) | psum (ct B)].  img_f, text_f_n and label
// are shared.  Floats of a row past e e + e are never addressed.
__global__ __launch_bounds__(64 * LP_WAVES) void lp_z_grouped_kernel(const float* __restrict__ x,
                                                                     const float* __restrict__ params, int64_t ps, float* z,
                                                                     int B, int e) {
  const int64_t s = blockIdx.z;
  const float* w = params + s * ps;
  lp_z_tile(x, w, w + (int64_t)e * e, z + s * B * e, B, e);
}

__global__ __launch_bounds__(64 * LP_WAVES) void lp_logits_grouped_kernel(const float* __restrict__ z,
                                                                          const float* __restrict__ t, float* logits,
                                                                          float* ws, int64_t wsf, float scale, int B, int C,
                                                                          int e) {
  const int64_t s = blockIdx.z;
  float* pmax = ws + s * wsf + (int64_t)B * e;
  lp_logits_tile(z + s * B * e, t, logits + s * B * C, pmax, pmax + (int64_t)((C + 31) / 32) * B, scale, B, C, e);
}

__global__ __launch_bounds__(64 * LP_WAVES) void lp_dz_grouped_kernel(const float* __restrict__ logits,
                                                                      const float* __restrict__ t, float* ws, int64_t wsf,
                                                                      const int64_t* __restrict__ label, float* loss,
                                                                      float gmul, int B, int C, int e) {
  const int64_t s = blockIdx.z;
  float* dz = ws + s * wsf;
  const float* pmax = dz + (int64_t)B * e;
  lp_dz_tile(logits + s * B * C, t, pmax, pmax + (int64_t)((C + 31) / 32) * B, label, dz, loss + s, gmul, B, C, e);
}

__global__ __launch_bounds__(64) void lp_gw_grouped_kernel(const float* __restrict__ ws, int64_t wsf,
                                                           const float* __restrict__ x, float* grads, int64_t ps, int B,
                                                           int e) {
  const int64_t s = blockIdx.z;
  float* g_w = grads + s * ps;
  lp_gw_tile(ws + s * wsf, x, g_w, g_w + (int64_t)e * e, B, e);
}

}  // namespace

extern "C" int64_t rpo_lp_head_workspace_floats(int B, int C, int e) {
  if (B <= 0 || C <= 0 || e <= 0) return 0;
  return (int64_t)B * e + 2 * (int64_t)((C + 31) / 32) * B;
}

extern "C" int rpo_lp_head_fwd_bwd(const float* img_f, const float* w, const float* bias, const float* text_f_n,
                                   const int64_t* label, float scale_exp, float* z, float* logits, float* loss,
                                   float* g_w, float* g_bias, int B, int C, int e, float* workspace, void* stream) {
  if (!img_f || !w || !bias || !text_f_n || !z || !logits || !workspace) return RPO_E_BADARG;
  if (label && (!loss || !g_w || !g_bias)) return RPO_E_BADARG;
  if (B < 1 || B > LP_MAX_B || C < 1 || C > LP_MAX_C || e < 32 || e > LP_MAX_E || e % 32 != 0) return RPO_E_SHAPE;
  if (!aligned16(img_f) || !aligned16(w) || !aligned16(z) || !aligned16(text_f_n)) return RPO_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int bt = (B + 31) / 32, ct = (C + 31) / 32, et = e / 32;
  float* dz = workspace;
  float* pmax = dz + (int64_t)B * e;
  float* psum = pmax + (int64_t)ct * B;
  hipLaunchKernelGGL(lp_z_kernel, dim3(et, bt), dim3(64 * LP_WAVES), 0, s, img_f, w, bias, z, B, e);
  hipLaunchKernelGGL(lp_logits_kernel, dim3(ct, bt), dim3(64 * LP_WAVES), 0, s, z, text_f_n, logits, pmax, psum, scale_exp,
                     B, C, e);
  if (!label) return rpo_launch_status();
  hipLaunchKernelGGL(lp_dz_kernel, dim3(et, bt), dim3(64 * LP_WAVES), 0, s, logits, text_f_n, pmax, psum, label, dz, loss,
                     scale_exp / (float)B, B, C, e);
  hipLaunchKernelGGL(lp_gw_kernel, dim3(et, et), dim3(64), 0, s, dz, img_f, g_w, g_bias, B, e);
  return rpo_launch_status();
}

extern "C" int rpo_lp_head_fwd_bwd_grouped(const float* img_f, const float* params, int64_t set_stride,
                                           const float* text_f_n, const int64_t* label, float scale_exp, float* z,
                                           float* logits, float* loss, float* grads, int S, int B, int C, int e,
                                           float* workspace, void* stream) {
  if (!img_f || !params || !text_f_n || !z || !logits || !workspace) return RPO_E_BADARG;
  if (label && (!loss || !grads)) return RPO_E_BADARG;
  if (B < 1 || B > LP_MAX_B || C < 1 || C > LP_MAX_C || e < 32 || e > LP_MAX_E || e % 32 != 0) return RPO_E_SHAPE;
  if (S < 1 || S > LP_MAX_S || set_stride < (int64_t)e * e + e) return RPO_E_SHAPE;
  if (set_stride % 4 != 0 || !aligned16(img_f) || !aligned16(params) || !aligned16(z) || !aligned16(text_f_n))
    return RPO_E_ALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int bt = (B + 31) / 32, ct = (C + 31) / 32, et = e / 32;
  const int64_t wsf = rpo_lp_head_workspace_floats(B, C, e);
  hipLaunchKernelGGL(lp_z_grouped_kernel, dim3(et, bt, S), dim3(64 * LP_WAVES), 0, st, img_f, params, set_stride, z, B, e);
  hipLaunchKernelGGL(lp_logits_grouped_kernel, dim3(ct, bt, S), dim3(64 * LP_WAVES), 0, st, z, text_f_n, logits, workspace,
                     wsf, scale_exp, B, C, e);
  if (!label) return rpo_launch_status();
  hipLaunchKernelGGL(lp_dz_grouped_kernel, dim3(et, bt, S), dim3(64 * LP_WAVES), 0, st, logits, text_f_n, workspace, wsf,
                     label, loss, scale_exp / (float)B, B, C, e);
  hipLaunchKernelGGL(lp_gw_grouped_kernel, dim3(et, et, S), dim3(64), 0, st, workspace, wsf, img_f, grads, set_stride,
                     B, e);
  return rpo_launch_status();
}
