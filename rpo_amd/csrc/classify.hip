// Classification of CACHED image features (rpo_amd/features.py): S classifiers over n resident feature rows in ONE launch --
// the cosine / affine head of the plain-tower trainers (trainers/zsclip.py:58-63, trainers/coop.py:196-208,
// trainers/linear_prob.py:85-95) fused with the evaluator of eval.hip, so that no logit has to reach memory:
//   logits[s,i,c] = a_i r_sc <feat[i,:], cls[s,c,:]> + bias[s,c],   a_i = scale (/ |feat[i,:]|),  r_sc = 1 (/ |cls[s,c,:]|)
//   pred[s,i] = the row maximum's index by eval.hip's rule; counts / confusion matrix as rpo_eval_accumulate sums them
//
// A workgroup owns (32 feature rows, classifier s).  It stages its rows in LDS once (row stride e + 4 floats: the 16-byte
// operand reads of 16 lanes then cover all 64 banks) and takes their norms from the staged copy.  Wave w walks the class
// tiles w, w + W, ...: one 32 x 32 accumulator tile over the WHOLE k range on the fp32 matrix pipe
// (v_mfma_f32_32x32x2_f32: exact fp32 products, one rounding per fma, k in the fixed order of lp_head.hip's lp_tile_nt),
// the classifier rows read straight from memory / L2 one 16-byte load ahead.  So an element's bits depend on its own
// feature row and classifier row alone -- not on the other rows, their number, the other classifiers or the wave count.
// Both norms are sums in double (fixed order), rounded once: (float)(scale / sqrt(sum)).  Every accumulator row keeps a
// running best (value, index); the rule is a total order (NaN first, larger value, lower index), so the merges across
// lanes and waves give the same result in any order.  Only integers are written (vector atomics), plus the optional
// logits_out.
#include "common.h"

namespace {

#ifndef FC_WAVES
#define FC_WAVES 8                             // waves per workgroup at most (-DFC_WAVES=...: the A/B of DESIGN.md 9n)
#endif
constexpr int FC_ROWS = 32, FC_PAD = 4, FC_MAX_WAVES = FC_WAVES;
constexpr int FC_MAX_E = 1024, FC_MAX_C = 65536, FC_MAX_S = 1024;

// acc[r] of v_mfma_f32_32x32x2_f32 is D[(r & 3) + 8 (r >> 2) + 4 half][l31] (lp_head.hip, rpo_probe_mfma)
__device__ __forceinline__ int fc_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// eval.hip's eval_better -- (v, i) is a strictly better prediction than (bv, bi); i == -1: nothing seen -- written without
// branches: the callers keep 16 running bests in registers and update them by selects
__device__ __forceinline__ bool fc_better(float v, int i, float bv, int bi) {
  const bool vn = v != v, bn = bv != bv;
  const bool by_value = vn ? !bn : (!bn & (v > bv));               // NaN beats every number, else the larger value
  const bool same = (vn & bn) | (v == bv);                          // ties, +-0, two NaN: the lower index
  return (i >= 0) & ((bi < 0) | by_value | (same & (i < bi)));
}

template <int EMAX, bool NORM_CLS>
__global__ __launch_bounds__(64 * FC_MAX_WAVES) void features_classify_kernel(
    const float* __restrict__ feat, int64_t ldf, const float* __restrict__ cls, const float* __restrict__ bias,
    const int64_t* __restrict__ label, float scale, int norm_feat, unsigned long long* counts, int32_t* cmat, int32_t* pred,
    float* logits_out, int n, int C, int e) {
  __shared__ __attribute__((aligned(16))) float s_feat[FC_ROWS * (EMAX + FC_PAD)];
  __shared__ float s_a[FC_ROWS];
  __shared__ float s_bv[FC_MAX_WAVES][FC_ROWS];
  __shared__ int s_bi[FC_MAX_WAVES][FC_ROWS];
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, half = lane >> 5, wv = tid >> 6, nw = blockDim.x >> 6;
  const int i0 = blockIdx.x * FC_ROWS, s = blockIdx.y;
  const int rows = min(FC_ROWS, n - i0);
  const int ld = e + FC_PAD;

  // ---- stage the rows (rows past n: zeros; their results are never written)
  if ((ldf & 3) == 0) {
    const int q4 = e >> 2;
    for (int idx = tid; idx < FC_ROWS * q4; idx += blockDim.x) {
      const int r = idx / q4, q = idx - r * q4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < rows) v = *reinterpret_cast<const float4*>(feat + (int64_t)(i0 + r) * ldf + 4 * q);
      *reinterpret_cast<float4*>(s_feat + r * ld + 4 * q) = v;
    }
  } else {                                                        // a leading dimension that breaks the 16-byte rows
    for (int idx = tid; idx < FC_ROWS * e; idx += blockDim.x) {
      const int r = idx / e, k = idx - r * e;
      s_feat[r * ld + k] = r < rows ? feat[(int64_t)(i0 + r) * ldf + k] : 0.f;
    }
  }
  __syncthreads();

  // ---- a_i: lane j sums elements j, j + 64, ... in double, then a butterfly (the same tree in every lane)
  for (int r = wv; r < FC_ROWS; r += nw) {
    float a = scale;
    if (norm_feat) {
      double acc = 0.0;
      for (int k = lane; k < e; k += 64) {
        const double v = (double)s_feat[r * ld + k];
        acc = fma(v, v, acc);
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
      a = (float)((double)scale / sqrt(acc));
    }
    if (lane == 0) s_a[r] = a;
  }
  __syncthreads();

  // ---- the class tiles of this wave
  float best_v[16];
  int best_i[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) { best_v[r] = 0.f; best_i[r] = -1; }
  const int ctiles = (C + 31) >> 5;
  const float* arow = s_feat + l31 * ld + 4 * half;
  for (int ct = wv; ct < ctiles; ct += nw) {
    const int c = ct * 32 + l31;
    const bool cok = c < C;
    const int64_t crow_i = (int64_t)s * C + min(c, C - 1);        // (a column past C reads the last row; never kept)
    const float* crow = cls + crow_i * e + 4 * half;
    f32x16_t d;
#pragma unroll
    for (int r = 0; r < 16; ++r) d[r] = 0.f;
    double q = 0.0;
    float4 bv = *reinterpret_cast<const float4*>(crow);
    for (int k = 0; k < e; k += 8) {                               // lane half h holds k .. k+7's elements 4h .. 4h+3
      const float4 av = *reinterpret_cast<const float4*>(arow + k);
      float4 bn = bv;
      if (k + 8 < e) bn = *reinterpret_cast<const float4*>(crow + k + 8);
      if (NORM_CLS) {
        q = fma((double)bv.x, (double)bv.x, q);
        q = fma((double)bv.y, (double)bv.y, q);
        q = fma((double)bv.z, (double)bv.z, q);
        q = fma((double)bv.w, (double)bv.w, q);
      }
      d = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, d, 0, 0, 0);
      d = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, d, 0, 0, 0);
      d = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, d, 0, 0, 0);
      d = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, d, 0, 0, 0);
      bv = bn;
    }
    float rs = 1.0f;
    if (NORM_CLS) {
      q += __shfl_xor(q, 32, 64);                                  // the two halves of the row: a + b in both lanes
      rs = (float)(1.0 / sqrt(q));
    }
    const float bj = bias ? bias[crow_i] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = fc_row(r, half);
      const float m = s_a[row] * rs;
      const float v = bias ? __fmaf_rn(d[r], m, bj) : d[r] * m;
      if (logits_out && cok && row < rows) logits_out[((int64_t)s * n + i0 + row) * C + c] = v;
      const bool take = cok & fc_better(v, c, best_v[r], best_i[r]);
      best_v[r] = take ? v : best_v[r];
      best_i[r] = take ? c : best_i[r];
    }
  }

  // ---- merge: the 32 lanes of a half (one class column each), then the waves
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float v = best_v[r];
    int i = best_i[r];
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {
      const float ov = __shfl_xor(v, o, 64);
      const int oi = __shfl_xor(i, o, 64);
      const bool take = fc_better(ov, oi, v, i);
      v = take ? ov : v;
      i = take ? oi : i;
    }
    if (l31 == 0) { s_bv[wv][fc_row(r, half)] = v; s_bi[wv][fc_row(r, half)] = i; }
  }
  __syncthreads();
  if (tid >= FC_ROWS) return;
  const bool valid = tid < rows;
  float v = s_bv[0][tid];
  int bi = s_bi[0][tid];
  for (int w = 1; w < nw; ++w) {
    const float wv_ = s_bv[w][tid];
    const int wi = s_bi[w][tid];
    const bool take = fc_better(wv_, wi, v, bi);
    v = take ? wv_ : v;
    bi = take ? wi : bi;
  }
  bool hit = false;
  if (valid) {
    const int i = i0 + tid;
    if (pred) pred[(int64_t)s * n + i] = bi;
    const int64_t lb = label[i];
    const bool ok = lb >= 0 && lb < C;            // a label outside [0, C): counted, never correct, no matrix cell
    hit = ok && lb == bi;
    if (cmat && ok) atomicAdd(cmat + ((int64_t)s * C + lb) * C + bi, 1);
  }
  const unsigned long long hits = __ballot(hit);
  if (tid == 0) {
    if (hits) atomicAdd(counts + 2 * s, (unsigned long long)__popcll(hits));
    atomicAdd(counts + 2 * s + 1, (unsigned long long)rows);
  }
}

template <int EMAX>
void fc_launch(dim3 grid, int waves, hipStream_t st, const float* feat, int64_t ldf, const float* cls, const float* bias,
               const int64_t* label, float scale, int norm_feat, int norm_cls, unsigned long long* counts, int32_t* cmat,
               int32_t* pred, float* logits_out, int n, int C, int e) {
  if (norm_cls)
    hipLaunchKernelGGL((features_classify_kernel<EMAX, true>), grid, dim3(64 * waves), 0, st, feat, ldf, cls, bias, label,
                       scale, norm_feat, counts, cmat, pred, logits_out, n, C, e);
  else
    hipLaunchKernelGGL((features_classify_kernel<EMAX, false>), grid, dim3(64 * waves), 0, st, feat, ldf, cls, bias, label,
                       scale, norm_feat, counts, cmat, pred, logits_out, n, C, e);
}

}  // namespace

extern "C" int rpo_features_classify(const float* feat, int64_t ldf, const float* cls, const float* bias,
                                     const int64_t* label, float scale, int norm_feat, int norm_cls, int64_t* counts,
                                     int32_t* cmat, int32_t* pred, float* logits_out, int n, int C, int e, int S,
                                     void* stream) {
  if (!feat || !cls || !label || !counts) return RPO_E_BADARG;
  if (n < 1 || C < 1 || C > FC_MAX_C || S < 1 || S > FC_MAX_S || e < 32 || e > FC_MAX_E || e % 32 != 0 || ldf < e)
    return RPO_E_SHAPE;
  if (!aligned16(feat) || !aligned16(cls) || reinterpret_cast<uintptr_t>(counts) % 8) return RPO_E_ALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int ctiles = (C + 31) / 32;
  int waves = 1;                                                                 // every wave has a class tile
  while (2 * waves <= FC_MAX_WAVES && 2 * waves <= ctiles) waves *= 2;
  const dim3 grid((n + FC_ROWS - 1) / FC_ROWS, S);
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
  if (e <= 256)
    fc_launch<256>(grid, waves, st, feat, ldf, cls, bias, label, scale, norm_feat, norm_cls, cnt, cmat, pred, logits_out, n, C, e);
  else if (e <= 512)
    fc_launch<512>(grid, waves, st, feat, ldf, cls, bias, label, scale, norm_feat, norm_cls, cnt, cmat, pred, logits_out, n, C, e);
  else
    fc_launch<1024>(grid, waves, st, feat, ldf, cls, bias, label, scale, norm_feat, norm_cls, cnt, cmat, pred, logits_out, n, C, e);
  return rpo_launch_status();
}
