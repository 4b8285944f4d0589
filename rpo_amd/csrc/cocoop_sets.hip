// CoCoOp for S independent runs ("members") of b images each in the launches of one (rpo_amd/coop_multi.py, DESIGN.md
// section 9r): the meta-net forward and backward with the member as a grid dimension, and the two elementwise ends of the
// step -- the shifted contexts in front of the text pass, the gradient tail behind it -- as one launch each.
//
// Member s owns row s of params / grads [S, set_stride]:
//   [ctx (n_ctx * d) | w1 (h * e) | b1 (h) | w2 (d * h) | b2 (d)]
// which is the flat buffer of a standalone run (engine_coop.coop_setup's coop_params), so a row can be copied into one and
// back.  Floats of a row past its length (the padding up to set_stride) are never read or written.
//
// The meta-net bodies are those of metanet_fwd_kernel / metanet_bwd_kernel (misc.hip) statement for statement -- only the
// addresses differ -- so an image / a member gets the bits of rpo_metanet_fwd / rpo_metanet_bwd(B = b) on its slices.  fp32,
// fixed summation orders, no atomics, no allocation: capturable in a HIP graph.
#include "common.h"

namespace {

struct RowLayout {
  int64_t ctx, w1, b1, w2, b2, len;
};
__host__ __device__ __forceinline__ RowLayout row_layout(int n_ctx, int e, int h, int d) {
  RowLayout r;
  r.ctx = 0;
  r.w1 = (int64_t)n_ctx * d;
  r.b1 = r.w1 + (int64_t)h * e;
  r.w2 = r.b1 + h;
  r.b2 = r.w2 + (int64_t)d * h;
  r.len = r.b2 + d;
  return r;
}

__device__ __forceinline__ float block_sum(float v, float* red) {  // 256 threads (misc.hip's)
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// One workgroup per (member, image): blockIdx.x = s * b + i reads member s's four tensors.
__global__ __launch_bounds__(256) void metanet_fwd_sets_kernel(const float* __restrict__ f, const float* __restrict__ params,
                                                               int64_t stride, int n_ctx, float* fn, float* hid, float* bias,
                                                               int b, int e, int h, int d) {
  extern __shared__ float mn_smem[];               // fn [e] | hid [h]
  __shared__ float red[4];
  float* sf = mn_smem;
  float* sh = mn_smem + e;
  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const RowLayout L = row_layout(n_ctx, e, h, d);
  const float* row = params + (int64_t)(img / b) * stride;
  const float* w1 = row + L.w1;
  const float* b1 = row + L.b1;
  const float* w2 = row + L.w2;
  const float* b2 = row + L.b2;
  float ss = 0.f;
  for (int i = tid; i < e; i += 256) { const float v = f[(int64_t)img * e + i]; ss = fmaf(v, v, ss); }
  ss = block_sum(ss, red);
  const float inv = 1.0f / sqrtf(ss);
  for (int i = tid; i < e; i += 256) {
    const float v = f[(int64_t)img * e + i] * inv;
    sf[i] = v;
    fn[(int64_t)img * e + i] = v;
  }
  __syncthreads();
  for (int j = wave; j < h; j += 4) {              // one wave per hidden unit: fixed-order lane partials + wave_sum
    float a = 0.f;
    for (int i = lane; i < e; i += 64) a = fmaf(w1[(int64_t)j * e + i], sf[i], a);
    a = wave_sum(a);
    if (lane == 0) {
      const float v = fmaxf(a + b1[j], 0.f);
      sh[j] = v;
      hid[(int64_t)img * h + j] = v;
    }
  }
  __syncthreads();
  for (int o = tid; o < d; o += 256) {
    float a = b2[o];
    for (int j = 0; j < h; ++j) a = fmaf(w2[(int64_t)o * h + j], sh[j], a);
    bias[(int64_t)img * d + o] = a;
  }
}

// c_shift[s * b + i, r, :] = ctx_s[r, :] + bias[s * b + i, :]  (trainers/cocoop.py:141-143), one element per thread.
__global__ __launch_bounds__(256) void cocoop_shift_sets_kernel(const float* __restrict__ params, int64_t stride,
                                                                const float* __restrict__ bias, float* __restrict__ shift,
                                                                int64_t total, int b, int n_ctx, int d) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int64_t per_img = (int64_t)n_ctx * d;
  const int64_t img = idx / per_img, k = idx - img * per_img;        // k = r * d + c
  const int c = (int)(k % d);
  shift[idx] = params[(img / b) * stride + k] + bias[img * d + c];
}

// The gradient tail of member s = blockIdx.y; output p of the member's n_ctx d + b d + 1:
//   p <  n_ctx d       : g_ctx_s[p]       = (1 / b) sum_i d_shift[s b + i, p]            i ascending
//   p <  n_ctx d + b d : d_bias[s b + i, c] = (1 / b) sum_r d_shift[s b + i, r, c]         r ascending
//   the last           : loss[s]          = (1 / b) sum_i loss_img[s b + i]              i ascending
// The sums start from their first term, so b = 1 returns d_shift and loss_img themselves.
__global__ __launch_bounds__(256) void cocoop_grad_tail_sets_kernel(const float* __restrict__ d_shift,
                                                                    const float* __restrict__ loss_img, float* grads,
                                                                    int64_t stride, float* __restrict__ d_bias,
                                                                    float* __restrict__ loss, int b, int n_ctx, int d) {
  const int s = blockIdx.y;
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t n_ctx_d = (int64_t)n_ctx * d, n_bias = (int64_t)b * d;
  const float inv_b = 1.0f / (float)b;
  const float* ds = d_shift + (int64_t)s * b * n_ctx_d;
  if (p < n_ctx_d) {
    float a = ds[p];
    for (int i = 1; i < b; ++i) a += ds[(int64_t)i * n_ctx_d + p];
    grads[(int64_t)s * stride + p] = a * inv_b;
  } else if (p < n_ctx_d + n_bias) {
    const int64_t q = p - n_ctx_d;
    const int i = (int)(q / d), c = (int)(q - (int64_t)i * d);
    const float* di = ds + (int64_t)i * n_ctx_d + c;
    float a = di[0];
    for (int r = 1; r < n_ctx; ++r) a += di[(int64_t)r * d];
    d_bias[((int64_t)s * b + i) * d + c] = a * inv_b;
  } else if (p == n_ctx_d + n_bias) {
    const float* li = loss_img + (int64_t)s * b;
    float a = li[0];
    for (int i = 1; i < b; ++i) a += li[i];
    loss[s] = a * inv_b;
  }
}

// metanet_bwd_kernel with the member as blockIdx.y: B = b images of member s, its w2, row s of grads.
__global__ __launch_bounds__(256) void metanet_bwd_sets_kernel(const float* __restrict__ dbias_all,
                                                               const float* __restrict__ fn_all,
                                                               const float* __restrict__ hid_all,
                                                               const float* __restrict__ params, float* grads, int64_t stride,
                                                               int n_ctx, int B, int e, int h, int d) {
  extern __shared__ float mn_smem[];               // dhid [B][h]
  const int tid = threadIdx.x, s = blockIdx.y;
  const RowLayout L = row_layout(n_ctx, e, h, d);
  const float* dbias = dbias_all + (int64_t)s * B * d;
  const float* fn = fn_all + (int64_t)s * B * e;
  const float* hid = hid_all + (int64_t)s * B * h;
  const float* w2 = params + (int64_t)s * stride + L.w2;
  float* grow = grads + (int64_t)s * stride;
  float* g_w1 = grow + L.w1;
  float* g_b1 = grow + L.b1;
  float* g_w2 = grow + L.w2;
  float* g_b2 = grow + L.b2;
  for (int p = tid; p < B * h; p += 256) {
    const int b = p / h, j = p - b * h;
    float a = 0.f;
    for (int o = 0; o < d; ++o) a = fmaf(dbias[(int64_t)b * d + o], w2[(int64_t)o * h + j], a);
    mn_smem[p] = hid[(int64_t)b * h + j] > 0.f ? a : 0.f;
  }
  __syncthreads();
  const int64_t idx = (int64_t)blockIdx.x * 256 + tid;
  const int64_t n_w2 = (int64_t)d * h, n_w1 = (int64_t)h * e;
  if (idx < n_w2) {
    const int o = (int)(idx / h), j = (int)(idx - (int64_t)o * h);
    float a = 0.f;
    for (int b = 0; b < B; ++b) a = fmaf(dbias[(int64_t)b * d + o], hid[(int64_t)b * h + j], a);
    g_w2[idx] = a;
  } else if (idx < n_w2 + n_w1) {
    const int64_t k = idx - n_w2;
    const int j = (int)(k / e), i = (int)(k - (int64_t)j * e);
    float a = 0.f;
    for (int b = 0; b < B; ++b) a = fmaf(mn_smem[b * h + j], fn[(int64_t)b * e + i], a);
    g_w1[k] = a;
  } else if (idx < n_w2 + n_w1 + d) {
    const int o = (int)(idx - n_w2 - n_w1);
    float a = 0.f;
    for (int b = 0; b < B; ++b) a += dbias[(int64_t)b * d + o];
    g_b2[o] = a;
  } else if (idx < n_w2 + n_w1 + d + h) {
    const int j = (int)(idx - n_w2 - n_w1 - d);
    float a = 0.f;
    for (int b = 0; b < B; ++b) a += mn_smem[b * h + j];
    g_b1[j] = a;
  }
}

constexpr int SETS_MAX_S = 1024;

// What all four entry points check of the member geometry: 0, or the error to return with nothing launched.  `need`: the
// floats of a row the call touches (the meta-net pair: the whole row; the two context-only calls: its ctx part).
int sets_check(int64_t set_stride, int64_t need, int S, int b) {
  if (S < 1 || S > SETS_MAX_S || b < 1 || (int64_t)S * b > 0x7fffffffLL) return RPO_E_SHAPE;
  if (set_stride < need) return RPO_E_SHAPE;
  if (set_stride % 4 != 0) return RPO_E_ALIGN;
  return 0;
}

}  // namespace

extern "C" int rpo_metanet_fwd_sets(const float* img_f, const float* params, int64_t set_stride, int n_ctx, float* f_norm,
                                    float* hidden, float* bias, int S, int b, int e, int h, int d, void* stream) {
  if (!img_f || !params || !f_norm || !hidden || !bias || n_ctx <= 0 || e <= 0 || h <= 0 || d <= 0) return RPO_E_BADARG;
  if (const int rc = sets_check(set_stride, row_layout(n_ctx, e, h, d).len, S, b)) return rc;
  if (((int64_t)e + h) * 4 > 48 * 1024) return RPO_E_SHAPE;
  if (!aligned16(params)) return RPO_E_ALIGN;
  hipLaunchKernelGGL(metanet_fwd_sets_kernel, dim3((unsigned)(S * b)), dim3(256), (e + h) * 4,
                     static_cast<hipStream_t>(stream), img_f, params, set_stride, n_ctx, f_norm, hidden, bias, b, e, h, d);
  return rpo_launch_status();
}

extern "C" int rpo_cocoop_shift_sets(const float* params, int64_t set_stride, const float* bias, float* c_shift, int S, int b,
                                     int n_ctx, int d, void* stream) {
  if (!params || !bias || !c_shift || n_ctx <= 0 || d <= 0) return RPO_E_BADARG;
  if (const int rc = sets_check(set_stride, (int64_t)n_ctx * d, S, b)) return rc;
  if (!aligned16(params)) return RPO_E_ALIGN;
  const int64_t total = (int64_t)S * b * n_ctx * d, blocks = (total + 255) / 256;
  if (blocks > 0x7fffffffLL) return RPO_E_SHAPE;
  hipLaunchKernelGGL(cocoop_shift_sets_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), params,
                     set_stride, bias, c_shift, total, b, n_ctx, d);
  return rpo_launch_status();
}

extern "C" int rpo_cocoop_grad_tail_sets(const float* d_shift, const float* loss_img, float* grads, int64_t set_stride,
                                         float* d_bias, float* loss, int S, int b, int n_ctx, int d, void* stream) {
  if (!d_shift || !loss_img || !grads || !d_bias || !loss || n_ctx <= 0 || d <= 0) return RPO_E_BADARG;
  if (const int rc = sets_check(set_stride, (int64_t)n_ctx * d, S, b)) return rc;
  if (!aligned16(grads)) return RPO_E_ALIGN;
  const int64_t outs = (int64_t)n_ctx * d + (int64_t)b * d + 1, blocks = (outs + 255) / 256;
  if (blocks > 0x7fffffffLL) return RPO_E_SHAPE;
  hipLaunchKernelGGL(cocoop_grad_tail_sets_kernel, dim3((unsigned)blocks, S), dim3(256), 0, static_cast<hipStream_t>(stream),
                     d_shift, loss_img, grads, set_stride, d_bias, loss, b, n_ctx, d);
  return rpo_launch_status();
}

extern "C" int rpo_metanet_bwd_sets(const float* d_bias, const float* f_norm, const float* hidden, const float* params,
                                    float* grads, int64_t set_stride, int n_ctx, int S, int b, int e, int h, int d,
                                    void* stream) {
  if (!d_bias || !f_norm || !hidden || !params || !grads || n_ctx <= 0 || e <= 0 || h <= 0 || d <= 0) return RPO_E_BADARG;
  if (const int rc = sets_check(set_stride, row_layout(n_ctx, e, h, d).len, S, b)) return rc;
  if ((int64_t)b * h * 4 > 48 * 1024) return RPO_E_SHAPE;
  if (!aligned16(params) || !aligned16(grads)) return RPO_E_ALIGN;
  const int64_t n = (int64_t)d * h + (int64_t)h * e + d + h;
  hipLaunchKernelGGL(metanet_bwd_sets_kernel, dim3((unsigned)((n + 255) / 256), S), dim3(256), b * h * 4,
                     static_cast<hipStream_t>(stream), d_bias, f_norm, hidden, params, grads, set_stride, n_ctx, b, e, h, d);
  return rpo_launch_status();
}
