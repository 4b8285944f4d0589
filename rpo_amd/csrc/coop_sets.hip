// CoOp for S runs ("members") with their OWN number of context vectors on one dense text pass (rpo_amd/coop_sweep.py,
// DESIGN.md section 9s): the two ends of that pass that know about members, one launch each.
//
// Member s owns row s of params / grads [S, set_stride]: its n_s = n_ctx_members[s] context vectors are the first n_s * d
// floats of the row (a standalone CoOp(n_ctx = n_s)'s flat coop_params), the floats up to n_max * d are its unused tail and
// the padding up to set_stride is never read or written.  The engine was built with the prompts of n_max placeholders;
// member s's prompts are those with delta = n_max - n_s placeholders removed, so its class-name tokens sit delta positions
// earlier and its sequences are delta shorter.  Rows are member-major: row ((s * n_cls + c) * L + p) is position p of class c
// of member s.
//
//   rpo_coop_fill_sets      the input rows of the text pass: [SOS | ctx_s | name . EOT | rest] + positional embedding, one
//                           fp32 add per element (what the host's float32 composition gives, bit for bit)
//   rpo_coop_ctx_grad_sets  row s of grads = the rows of the context positions of dx summed over the classes, in the order
//                           of rpo_reduce_groups(groups = n_cls, rows = n_s) (misc.hip: one thread per element below 64
//                           groups, eight partial sums per element from 64 on), read in place; the unused tail is zeroed
//
// n_ctx_members is DEVICE data (int32 [S]); a value outside [0, n_max] is clamped into it, so no value makes either kernel
// read or write out of bounds.  fp32, no atomics, fixed summation orders, no allocation: capturable in a HIP graph.
#include "common.h"

namespace {

constexpr int SETS_MAX_S = 1024;

__device__ __forceinline__ int member_n_ctx(const int32_t* __restrict__ n_ctx_members, int s, int n_max) {
  return min(max(n_ctx_members[s], 0), n_max);
}

// One workgroup per row (s, c, p); d4 = d / 4 float4 per row.
__global__ __launch_bounds__(128) void coop_fill_sets_kernel(const float4* __restrict__ tok, const float4* __restrict__ pos,
                                                             const float* __restrict__ params, int64_t stride,
                                                             const int32_t* __restrict__ n_ctx_members,
                                                             float4* __restrict__ x0, int n_cls, int L, int n_max, int d4) {
  const int64_t row = blockIdx.x;
  const int64_t sc = row / L;
  const int p = (int)(row - sc * L);
  const int s = (int)(sc / n_cls), c = (int)(sc - (int64_t)s * n_cls);
  const int n_s = member_n_ctx(n_ctx_members, s, n_max);
  const int delta = n_max - n_s;
  const float4* src = nullptr;                       // nullptr: past the shortened prompt -- the positional embedding alone
  if (p == 0) src = tok + (int64_t)c * L * d4;
  else if (p <= n_s) src = reinterpret_cast<const float4*>(params + (int64_t)s * stride) + (int64_t)(p - 1) * d4;
  else if (p + delta < L) src = tok + ((int64_t)c * L + p + delta) * d4;
  const float4* pe = pos + (int64_t)p * d4;
  float4* o = x0 + row * d4;
  for (int i = threadIdx.x; i < d4; i += 128) {
    const float4 b = pe[i];
    if (src) {
      const float4 a = src[i];
      o[i] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
    } else {
      o[i] = b;
    }
  }
}

// reduce_groups_kernel (misc.hip) with the member as blockIdx.y, reading the context rows of dx in place: element idx =
// i * d + c of the row's first n_max * d floats is the sum over the classes g = 0, 1, .. of dx[(s, g, 1 + i), c], starting
// from 0.f as that kernel does; i >= n_s: an exact zero.
__global__ __launch_bounds__(256) void coop_ctx_grad_sets_kernel(const float* __restrict__ dx, float* __restrict__ grads,
                                                                 int64_t stride, const int32_t* __restrict__ n_ctx_members,
                                                                 int n_cls, int L, int n_max, int d) {
  const int s = blockIdx.y;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= n_max * d) return;
  const int i = idx / d, c = idx % d;
  float a = 0.f;
  if (i < member_n_ctx(n_ctx_members, s, n_max)) {
    const float* src = dx + ((int64_t)s * n_cls * L + 1 + i) * d + c;
    for (int g = 0; g < n_cls; ++g) a += src[(int64_t)g * L * d];
  }
  grads[(int64_t)s * stride + idx] = a;
}

// reduce_groups_wide_kernel (misc.hip) the same way: a block of 256 threads owns 32 consecutive columns of context row i and
// splits the classes over its 8 thread rows (thread row j sums classes j, j + 8, .. in ascending order), then adds the 8
// partial sums in thread-row order.
__global__ __launch_bounds__(256) void coop_ctx_grad_sets_wide_kernel(const float* __restrict__ dx, float* __restrict__ grads,
                                                                      int64_t stride,
                                                                      const int32_t* __restrict__ n_ctx_members, int n_cls,
                                                                      int L, int n_max, int d) {
  __shared__ float part[8][32];
  const int s = blockIdx.y;
  const int cols = (d + 31) / 32;
  const int i = blockIdx.x / cols, c = (blockIdx.x % cols) * 32 + (threadIdx.x & 31), j = threadIdx.x >> 5;
  const bool live = i < member_n_ctx(n_ctx_members, s, n_max);                   // (the same for the whole block)
  float a = 0.f;
  if (live && c < d) {
    const float* src = dx + ((int64_t)s * n_cls * L + 1 + i) * d + c;
    for (int g = j; g < n_cls; g += 8) a += src[(int64_t)g * L * d];
  }
  part[j][threadIdx.x & 31] = a;
  __syncthreads();
  if (j == 0 && c < d) {
    float t = part[0][threadIdx.x];
#pragma unroll
    for (int k = 1; k < 8; ++k) t += part[k][threadIdx.x];
    grads[(int64_t)s * stride + (int64_t)i * d + c] = live ? t : 0.f;
  }
}

// What both entry points check of the geometry: 0, or the error to return with nothing launched.
int coop_sets_check(int64_t set_stride, int S, int n_cls, int L, int n_max, int d) {
  if (n_cls <= 0 || L <= 0 || d <= 0) return RPO_E_BADARG;
  if (S < 1 || S > SETS_MAX_S || n_max < 1 || n_max + 1 > L) return RPO_E_SHAPE;
  if ((int64_t)n_max * d > 0x7fffffffLL || set_stride < (int64_t)n_max * d) return RPO_E_SHAPE;
  if ((int64_t)S * n_cls * L > 0x7fffffffLL) return RPO_E_SHAPE;
  if (set_stride % 4 != 0) return RPO_E_ALIGN;
  return 0;
}

}  // namespace

extern "C" int rpo_coop_fill_sets(const float* tok, const float* pos, const float* params, int64_t set_stride,
                                  const int32_t* n_ctx_members, float* x0, int S, int n_cls, int L, int n_max, int d,
                                  void* stream) {
  if (!tok || !pos || !params || !n_ctx_members || !x0) return RPO_E_BADARG;
  if (const int rc = coop_sets_check(set_stride, S, n_cls, L, n_max, d)) return rc;
  if (d % 4 != 0) return RPO_E_SHAPE;
  if (!aligned16(tok) || !aligned16(pos) || !aligned16(params) || !aligned16(x0)) return RPO_E_ALIGN;
  const int64_t rows = (int64_t)S * n_cls * L;
  hipLaunchKernelGGL(coop_fill_sets_kernel, dim3((unsigned)rows), dim3(128), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const float4*>(tok), reinterpret_cast<const float4*>(pos), params, set_stride,
                     n_ctx_members, reinterpret_cast<float4*>(x0), n_cls, L, n_max, d / 4);
  return rpo_launch_status();
}

extern "C" int rpo_coop_ctx_grad_sets(const float* dx, float* grads, int64_t set_stride, const int32_t* n_ctx_members, int S,
                                      int n_cls, int L, int n_max, int d, void* stream) {
  if (!dx || !grads || !n_ctx_members) return RPO_E_BADARG;
  if (const int rc = coop_sets_check(set_stride, S, n_cls, L, n_max, d)) return rc;
  if (!aligned16(grads)) return RPO_E_ALIGN;
  if (n_cls >= 64)           // (rpo_reduce_groups's own threshold between its two summation orders)
    hipLaunchKernelGGL(coop_ctx_grad_sets_wide_kernel, dim3(n_max * ((d + 31) / 32), S), dim3(256), 0,
                       static_cast<hipStream_t>(stream), dx, grads, set_stride, n_ctx_members, n_cls, L, n_max, d);
  else
    hipLaunchKernelGGL(coop_ctx_grad_sets_kernel, dim3((n_max * d + 255) / 256, S), dim3(256), 0,
                       static_cast<hipStream_t>(stream), dx, grads, set_stride, n_ctx_members, n_cls, L, n_max, d);
  return rpo_launch_status();
}
