// rpo_optim_step_sets: torch.optim's SGD (with dampening / Nesterov), Adam, AdamW, AMSGrad and RMSprop for `sets` runs in one
// launch, every setting that changes between steps or epochs read from device tables (include/rpo_amd.h, DESIGN.md
// section 9k).  It generalises rpo_sgd_step_sets (misc.hip): the same two forms (elementwise / one guarded 1024-thread
// workgroup per set), the same `used` and `found_inf` semantics, and for kind SGD with dampening 0 and no Nesterov the
// same instructions per element.
//
// Rules: torch/optim/{sgd,adam,adamw,rmsprop}.py, single-tensor path, not capturable, maximize = False.  torch forms the
// scalars of a step (1 - beta, 1 - beta^t, lr / bc1, sqrt(bc2), 1 - lr wd) in Python doubles and rounds each to fp32 once
// when it meets a tensor; here thread 0 of a workgroup forms them in double once per launch and hands them to the others
// through LDS (set_consts).  The two betas / alpha / dampening arrive as hi + lo float pairs: fp32(0.999) alone is
// 1.3e-5 away from 0.999 relative to 1 - beta2, which is the first step's whole bias correction.
#include "common.h"

namespace {

struct SetConsts {
  int kind;                          // RPO_OPT_* or -1: the set is ignored
  int first;                         // step[s] == 0
  float lr, gs, wd, c3, c4, eps;     // c3 = momentum / beta1, c4 = dampening / beta2 / alpha (their fp32 roundings)
  float om3, om4;                    // (float)(1 - beta1), (float)(1 - dampening | beta2 | alpha)
  float step_size, bc2_sqrt, decay;  // Adam kinds: lr / bc1, sqrt(bc2); AdamW: 1 - lr wd
  int nesterov, plain;               // SGD: Nesterov flag; dampening == 0 exactly
};

__device__ __forceinline__ void set_consts(SetConsts& c, const int32_t* __restrict__ kind, const float* __restrict__ hyper,
                                           const int32_t* __restrict__ step, int set, bool have_s2) {
  const float* h = hyper + 8 * set;
  const int k = kind[set];
  const int t0 = step[set];
  c.kind = (k < RPO_OPT_SGD || k > RPO_OPT_RMSPROP || t0 < 0 || (k == RPO_OPT_AMSGRAD && !have_s2)) ? -1 : k;
  c.first = t0 == 0;
  c.lr = h[0]; c.gs = h[1]; c.wd = h[2]; c.c3 = h[3]; c.c4 = h[4]; c.eps = h[5];
  const bool adam = k == RPO_OPT_ADAM || k == RPO_OPT_ADAMW || k == RPO_OPT_AMSGRAD;
  const double b1 = (double)h[3] + (adam ? (double)h[6] : 0.0);
  const double b2 = (double)h[4] + (double)h[7];
  c.om3 = (float)(1.0 - b1);
  c.om4 = (float)(1.0 - b2);
  c.nesterov = !adam && h[6] != 0.f;
  c.plain = h[4] == 0.f && h[7] == 0.f;
  c.step_size = c.lr; c.bc2_sqrt = 1.f;
  if (adam) {
    const double t = (double)t0 + 1.0;                      // the counter after this step
    c.step_size = (float)((double)h[0] / (1.0 - pow(b1, t)));
    c.bc2_sqrt = (float)sqrt(1.0 - pow(b2, t));
  }
  c.decay = (float)(1.0 - (double)h[0] * (double)h[2]);
}

// One element.  Contraction is OFF in this function and every fma is written out, so that the rounding sequence is this
// source's and not the optimiser's choice:
//  - kind SGD with dampening 0 and Nesterov off is what hipcc makes of sgd_kernel (misc.hip): two rounded products (one
//    v_pk_mul_f32) and a rounded sum for g', then fma(mom, buf, g') and fma(-lr, buf, p) -- that kernel's bits.  (The same
//    source expression left to contract inside this larger function came out differently in the last bit of buf.)
//  - everything else follows the forms of torch's CPU kernels: add(alpha) = fma(alpha, b, a), lerp = fma(w, b - a, a),
//    addcmul = fma(value * t1, t2, a), addcdiv = a + (value * t1) / t2, mul_ then add_ = fma(alpha, b, round(mul)).
__device__ __forceinline__ void optim_element(const SetConsts& c, float* p, const float* __restrict__ g, float* s0, float* s1,
                                              float* s2, int64_t i) {
#pragma clang fp contract(off)
  const float pi = p[i];
  if (c.kind == RPO_OPT_SGD) {
    const float lr = c.lr, mom = c.c3, wd = c.wd, gs = c.gs;
    const bool plain = c.plain && !c.nesterov;
    const float gi = plain ? gs * g[i] + wd * pi : __builtin_fmaf(wd, pi, gs * g[i]);
    float bi = gi;
    if (!c.first) bi = c.plain ? __builtin_fmaf(mom, s0[i], gi) : __builtin_fmaf(c.om4, gi, mom * s0[i]);
    s0[i] = bi;
    p[i] = __builtin_fmaf(-lr, c.nesterov ? __builtin_fmaf(mom, bi, gi) : bi, pi);
  } else if (c.kind == RPO_OPT_RMSPROP) {
    const float gi = __builtin_fmaf(c.wd, pi, c.gs * g[i]);
    const float sq = __builtin_fmaf(c.om4 * gi, gi, c.c4 * s1[i]);
    s1[i] = sq;
    const float a = sqrtf(sq) + c.eps;
    if (c.c3 > 0.f) {
      const float bi = c.c3 * s0[i] + gi / a;
      s0[i] = bi;
      p[i] = __builtin_fmaf(-c.lr, bi, pi);
    } else {
      p[i] = pi + (-c.lr * gi) / a;
    }
  } else {                                                  // ADAM / ADAMW / AMSGRAD
    float pw = pi, gi = c.gs * g[i];
    if (c.kind == RPO_OPT_ADAMW) pw = pi * c.decay;
    else gi = __builtin_fmaf(c.wd, pi, gi);
    const float m0 = s0[i];
    const float m = __builtin_fmaf(c.om3, gi - m0, m0);     // lerp_(grad, 1 - beta1), weight < 0.5
    float v = __builtin_fmaf(c.om4 * gi, gi, c.c4 * s1[i]);
    s0[i] = m; s1[i] = v;
    if (c.kind == RPO_OPT_AMSGRAD) { v = fmaxf(s2[i], v); s2[i] = v; }
    const float denom = sqrtf(v) / c.bc2_sqrt + c.eps;
    p[i] = pw + (-c.step_size * m) / denom;
  }
}

__device__ __forceinline__ bool set_uses(int64_t i, int64_t seg0, int64_t u0, int64_t u1) {
  return i < seg0 ? i < u0 : i - seg0 < u1;
}
__device__ __forceinline__ void set_ranges(const int32_t* used, int set, int64_t seg0, int64_t seg1, int64_t& u0, int64_t& u1) {
  u0 = seg0; u1 = seg1;
  if (used != nullptr) {
    u0 = min(max((int64_t)used[2 * set], (int64_t)0), seg0);
    u1 = min(max((int64_t)used[2 * set + 1], (int64_t)0), seg1);
  }
}

// Elementwise form: blockIdx.y = set, many workgroups per set.  Every workgroup READS step[set]; nobody in this launch
// writes it (optim_advance_kernel does, behind this launch on the same stream).
__global__ __launch_bounds__(256) void optim_sets_kernel(float* p, const float* __restrict__ g, float* s0, float* s1, float* s2,
                                                         int64_t set_stride, const int32_t* __restrict__ kind,
                                                         const float* __restrict__ hyper, const int32_t* __restrict__ step,
                                                         const int32_t* __restrict__ used, int64_t seg0, int64_t seg1) {
  __shared__ SetConsts c;
  const int set = blockIdx.y;
  if (threadIdx.x == 0) set_consts(c, kind, hyper, step, set, s2 != nullptr);
  __syncthreads();
  if (c.kind < 0) return;
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= seg0 + seg1) return;
  int64_t u0, u1;
  set_ranges(used, set, seg0, seg1, u0, u1);
  if (!set_uses(j, seg0, u0, u1)) return;
  const int64_t off = (int64_t)set * set_stride;
  optim_element(c, p + off, g + off, s0 + off, s1 + off, s2 ? s2 + off : nullptr, j);
}

__global__ void optim_advance_kernel(const int32_t* __restrict__ kind, int32_t* step, int sets, int have_s2) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= sets) return;
  const int k = kind[s], t = step[s];
  if (k < RPO_OPT_SGD || k > RPO_OPT_RMSPROP || t < 0 || (k == RPO_OPT_AMSGRAD && !have_s2)) return;
  if (t < 0x7fffffff) step[s] = t + 1;
}

// Guarded form: one workgroup per set, so the set's counter has one reader-writer (thread 0, read before the scan, written
// after the update).
__global__ __launch_bounds__(1024) void optim_sets_guarded_kernel(float* p, const float* __restrict__ g, float* s0, float* s1,
                                                                  float* s2, int64_t set_stride,
                                                                  const int32_t* __restrict__ kind,
                                                                  const float* __restrict__ hyper, int32_t* step,
                                                                  const int32_t* __restrict__ used, int64_t seg0,
                                                                  int64_t seg1, int32_t* found) {
  __shared__ SetConsts c;
  __shared__ int bad;
  const int set = blockIdx.x;
  const int64_t off = (int64_t)set * set_stride;
  p += off; g += off; s0 += off; s1 += off; if (s2) s2 += off;
  found += 2 * set;
  int64_t u0, u1;
  set_ranges(used, set, seg0, seg1, u0, u1);
  const int64_t n = seg0 + seg1;
  if (threadIdx.x == 0) { bad = 0; set_consts(c, kind, hyper, step, set, s2 != nullptr); }
  __syncthreads();
  if (c.kind < 0) return;                                   // an ignored set: nothing scanned, nothing written
  int mine = 0;
  for (int64_t i = threadIdx.x; i < n; i += 1024) {
    if (!set_uses(i, seg0, u0, u1)) continue;
    const float gi = g[i];
    mine |= !(fabsf(gi) <= 3.402823466e38f);                // Inf or NaN
  }
  if (mine) bad = 1;
  __syncthreads();
  const int skip = bad;
  if (threadIdx.x == 0) {
    found[0] = skip; found[1] += skip;
    if (!skip) { const int t = step[set]; if (t < 0x7fffffff) step[set] = t + 1; }
  }
  if (skip) return;
  for (int64_t i = threadIdx.x; i < n; i += 1024) {
    if (!set_uses(i, seg0, u0, u1)) continue;
    optim_element(c, p, g, s0, s1, s2, i);
  }
}

}  // namespace

extern "C" int rpo_optim_step_sets(float* p, const float* g, float* s0, float* s1, float* s2, int64_t set_stride, int sets,
                                   const int32_t* kind, const float* hyper, int32_t* step, const int32_t* used, int64_t seg0,
                                   int64_t seg1, int needs_s2, int32_t* found_inf, void* stream) {
  if (!p || !g || !s0 || !s1 || !kind || !hyper || !step || sets <= 0 || seg0 < 0 || seg1 < 0 || (seg0 == 0 && seg1 == 0))
    return RPO_E_BADARG;
  if (needs_s2 && !s2) return RPO_E_BADARG;
  if (seg0 > INT64_MAX - seg1) return RPO_E_SHAPE;          // (the sum below would overflow)
  if (set_stride < seg0 + seg1 || sets > 65535) return RPO_E_SHAPE;
  if (seg0 + seg1 > (int64_t)0x7fffffff * 256) return RPO_E_SHAPE;      // (grid.x of the elementwise form)
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (found_inf) {
    hipLaunchKernelGGL(optim_sets_guarded_kernel, dim3(sets), dim3(1024), 0, st, p, g, s0, s1, s2, set_stride, kind, hyper,
                       step, used, seg0, seg1, found_inf);
  } else {
    hipLaunchKernelGGL(optim_sets_kernel, dim3((unsigned)((seg0 + seg1 + 255) / 256), sets), dim3(256), 0, st, p, g, s0, s1,
                       s2, set_stride, kind, hyper, step, used, seg0, seg1);
    hipLaunchKernelGGL(optim_advance_kernel, dim3((unsigned)((sets + 255) / 256)), dim3(256), 0, st, kind, step, sets,
                       s2 != nullptr);
  }
  return rpo_launch_status();
}
