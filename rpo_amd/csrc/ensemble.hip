// Prompt ensembling (trainers/zsclip.py:85-96, ZeroshotCLIP2): the classifier is the normalised mean over T templates of
// the normalised text features of every class.
//   accumulate: acc[c,:] = (first ? 0 : acc[c,:]) + sum_t feat[t,c,:] / ||feat[t,c,:]||      (:88-94)
//   finish:     out[c,:] = m / ||m||,  m = acc[c,:] / T_total                                (:95-96)
// All fp32.  One wave owns one class row (e <= 1024: at most 16 floats per lane, held in registers): a pass for the norm,
// a pass for the scaled add, the templates one after the other in ascending t.  No atomics, nothing crosses a wave, so the
// bits repeat from call to call, and because the running sum goes through `acc` unrounded (fp32 in, fp32 out) a call over T
// templates gives the bits of a call over the first T1 followed by a call over the rest.
// Two element maps: 16-byte loads (lane j holds floats 4 (j + 64 i) .. + 3) where e, the leading dimensions and the base
// addresses allow it, else one float per load (lane j holds floats j + 64 i).  The map fixes the order of the norm's sum;
// it depends on (e, ld, alignment) only, never on T, n_cls or `first`.
#include "common.h"

namespace {

constexpr int ENS_WAVES = 4;                    // class rows per workgroup
constexpr int ENS_MAX_E = 1024;                 // the head's limit (misc.hip)

// VEC: 4 x float4 per lane; else 16 x float per lane.  `n` = e / 4 or e.
template <bool VEC> struct EnsRow {
  static constexpr int N = VEC ? 4 : 16;
  float v[16];

  __device__ __forceinline__ void load(const float* __restrict__ p, int n, int lane) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int j = lane + 64 * i;
      if (VEC) {
        const float4 x = j < n ? *reinterpret_cast<const float4*>(p + 4 * j) : make_float4(0.f, 0.f, 0.f, 0.f);
        v[4 * i] = x.x; v[4 * i + 1] = x.y; v[4 * i + 2] = x.z; v[4 * i + 3] = x.w;
      } else {
        v[i] = j < n ? p[j] : 0.f;
      }
    }
  }
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = 0.f;
  }
  __device__ __forceinline__ void store(float* p, int n, int lane) const {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int j = lane + 64 * i;
      if (j >= n) continue;
      if (VEC) *reinterpret_cast<float4*>(p + 4 * j) = make_float4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
      else p[j] = v[i];
    }
  }
  // ||row||_2: the lane's squares in register order, then the butterfly over the wave (the same value in every lane)
  __device__ __forceinline__ float norm() const {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) s = fmaf(v[i], v[i], s);
    return sqrtf(wave_sum(s));
  }
};

template <bool VEC>
__global__ __launch_bounds__(64 * ENS_WAVES) void ens_accumulate_kernel(const float* __restrict__ feat, int64_t ld, int T,
                                                                        int64_t tstride, int n_cls, int e, float* acc,
                                                                        int first) {
  const int lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * ENS_WAVES + (threadIdx.x >> 6);
  if (c >= n_cls) return;                                          // (whole waves: no barrier follows)
  const int n = VEC ? e / 4 : e;
  EnsRow<VEC> a, f;
  if (first) a.zero();
  else a.load(acc + c * e, n, lane);
  for (int t = 0; t < T; ++t) {                                    // ascending t: zsclip.py:89-94
    f.load(feat + ((int64_t)t * tstride + c) * ld, n, lane);
    const float nrm = f.norm();
#pragma unroll
    for (int i = 0; i < 16; ++i) a.v[i] += f.v[i] / nrm;
  }
  a.store(acc + c * e, n, lane);
}

template <bool VEC>
__global__ __launch_bounds__(64 * ENS_WAVES) void ens_finish_kernel(const float* acc, int n_cls, int e, float t_total,
                                                                    float* out) {
  const int lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * ENS_WAVES + (threadIdx.x >> 6);
  if (c >= n_cls) return;
  const int n = VEC ? e / 4 : e;
  EnsRow<VEC> m;
  m.load(acc + c * e, n, lane);                                    // the whole row is in registers before any store:
#pragma unroll                                                     // out may alias acc
  for (int i = 0; i < 16; ++i) m.v[i] = m.v[i] / t_total;
  const float nrm = m.norm();
#pragma unroll
  for (int i = 0; i < 16; ++i) m.v[i] = m.v[i] / nrm;
  m.store(out + c * e, n, lane);
}

}  // namespace

extern "C" int rpo_text_ensemble_accumulate(const float* feat, int64_t ld, int T, int64_t template_stride_rows, int n_cls,
                                            int e, float* acc, int first, void* stream) {
  if (!feat || !acc || T < 1 || n_cls < 1 || e < 1 || e > ENS_MAX_E || ld < e || (T > 1 && template_stride_rows < n_cls))
    return RPO_E_BADARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((n_cls + ENS_WAVES - 1) / ENS_WAVES), block(64 * ENS_WAVES);
  if (e % 4 == 0 && ld % 4 == 0 && aligned16(feat) && aligned16(acc))
    hipLaunchKernelGGL(ens_accumulate_kernel<true>, grid, block, 0, s, feat, ld, T, template_stride_rows, n_cls, e, acc, first);
  else
    hipLaunchKernelGGL(ens_accumulate_kernel<false>, grid, block, 0, s, feat, ld, T, template_stride_rows, n_cls, e, acc, first);
  return rpo_launch_status();
}

extern "C" int rpo_text_ensemble_finish(const float* acc, int n_cls, int e, int T_total, float* out, void* stream) {
  if (!acc || !out || T_total < 1 || n_cls < 1 || e < 1 || e > ENS_MAX_E) return RPO_E_BADARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((n_cls + ENS_WAVES - 1) / ENS_WAVES), block(64 * ENS_WAVES);
  if (e % 4 == 0 && aligned16(acc) && aligned16(out))
    hipLaunchKernelGGL(ens_finish_kernel<true>, grid, block, 0, s, acc, n_cls, e, (float)T_total, out);
  else
    hipLaunchKernelGGL(ens_finish_kernel<false>, grid, block, 0, s, acc, n_cls, e, (float)T_total, out);
  return rpo_launch_status();
}
