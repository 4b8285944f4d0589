// Classification evaluator on the device (Dassl's `Classification` evaluator, `compute_accuracy` of the CoOp / LP steps):
// per image the prediction `logits.max(1)[1]`, and integer sums -- correct / total and the confusion matrix -- that
// ACCUMULATE in caller-owned device buffers, so an epoch or a test pass reads them back once.
//
// One wave per image.  A lane scans classes lane, lane + 64, ... and keeps the first best it meets; a butterfly then
// merges the 64 candidates.  "Best" is torch's CPU order for fp32: NaN beats every number, otherwise the larger value,
// and among equals (ties, +-0, several NaN) the lower index.  The sums are integers added with vector global atomics, so
// every order of arrival gives the same bits.
#include "common.h"

namespace {

constexpr int EVAL_MAX_B = 65536, EVAL_MAX_C = 65536;

// (v, i) is a strictly better prediction than (bv, bi).  A lane that has seen nothing holds i == -1.
__device__ __forceinline__ bool eval_better(float v, int i, float bv, int bi) {
  if (i < 0) return false;
  if (bi < 0) return true;
  const bool vn = v != v, bn = bv != bv;
  if (vn != bn) return vn;
  if (!vn && v != bv) return v > bv;
  return i < bi;
}

__global__ __launch_bounds__(64) void eval_accumulate_kernel(const float* __restrict__ logits, int64_t ldl,
                                                             const int64_t* __restrict__ label, int C,
                                                             unsigned long long* counts, int32_t* cmat, int32_t* pred) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const float* row = logits + (int64_t)b * ldl;
  float bv = 0.f;
  int bi = -1;
  for (int c = lane; c < C; c += 64) {            // ascending c: a later equal never replaces an earlier one
    const float v = row[c];
    if (eval_better(v, c, bv, bi)) { bv = v; bi = c; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (eval_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  if (lane != 0) return;
  if (pred) pred[b] = bi;
  const int64_t lb = label[b];
  const bool ok = lb >= 0 && lb < C;              // a label outside [0, C): counted, never correct, no matrix cell
  if (ok && lb == bi) atomicAdd(counts, 1ull);
  atomicAdd(counts + 1, 1ull);
  if (cmat && ok) atomicAdd(cmat + lb * C + bi, 1);
}

}  // namespace

extern "C" int rpo_eval_accumulate(const float* logits, int64_t ldl, const int64_t* label, int B, int C,
                                   int64_t* counts, int32_t* cmat, int32_t* pred, void* stream) {
  if (!logits || !label || !counts) return RPO_E_BADARG;
  if (B < 1 || B > EVAL_MAX_B || C < 1 || C > EVAL_MAX_C || ldl < C) return RPO_E_SHAPE;
  if (reinterpret_cast<uintptr_t>(counts) % 8) return RPO_E_ALIGN;
  hipLaunchKernelGGL(eval_accumulate_kernel, dim3(B), dim3(64), 0, static_cast<hipStream_t>(stream), logits, ldl, label,
                     C, reinterpret_cast<unsigned long long*>(counts), cmat, pred);
  return rpo_launch_status();
}
