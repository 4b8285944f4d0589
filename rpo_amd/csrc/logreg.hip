// CLIP's linear-probe protocol on CACHED image features (rpo_amd/logreg.py): S L2-regularised multinomial
// logistic regressions -- the members of a regularisation / few-shot sweep -- over one resident feature matrix.  Member s:
//   z_sic = a_i <f_i, W_s[c,:]> + b_s[c]                 (rpo_features_classify's logits with scale 1, norm_cls 0)
//   J_s   = (1/Omega_s) sum_i w_si CE(softmax(z_si.), y_i) + (l2[s]/2) |W_s|_F^2,     Omega_s = sum_i w_si
// rpo_logreg_loss_grad_sets is three launches, the member a grid dimension in each:
//   lg_fwd:   workgroup = (32 feature rows, member), classify.hip's scaffold: the rows staged in LDS once, a_i from the staged
//             copy (double sum, rounded once), wave w walks the class tiles w, w + W, ... with one 32 x 32 accumulator over
//             the whole k range (v_mfma_f32_32x32x2_f32: exact fp32 products, one rounding per fma, fixed k order).  The
//             32 x C logit tile goes THROUGH THE WORKSPACE, not LDS: at e = 1024 the staged rows are 128.5 KiB of the CU's
//             160 KiB and a 32 x 1024 fp32 logit tile would be another 128 KiB; the residual matrix R has to be written to
//             memory anyway (the gradient launch reads it), so the logits take R's place and the same workgroup reads them
//             back (from its own L1 / L2) one wave per row: row max in fp32, sum of exp, p, the weight and the division by
//             Omega in double, ONE rounding into r_sic = (w_si / Omega_s)(p_sic - [c == y_i]).  Per tile one fp32 loss
//             partial (a double sum in row order, rounded once).  The workgroups of tile 0 also form (l2/2)|W_s|^2 from the
//             classifier rows they stream anyway (double, fixed order).
//   lg_grad:  G_s = R_s^T (a . F) as a GEMM reduced over n in chunks of LG_CHUNK rows: wave = (32 classes, 32 NB features,
//             chunk), rows in ascending order on the same matrix pipe; both operands are read row by row, coalesced.  The
//             waves of feature block 0 also sum their R columns (the bias gradient's partial).  fp32 partials
//             [S, chunks, C, e] / [S, chunks, C].
//   lg_final: workgroup = (class row, member): the partials in ascending chunk order, + l2[s] W_s; the bias gradient; the
//             workgroup of class 0 adds the loss partials in ascending tile order (double, rounded once) and the penalty.
// No float atomics anywhere: the bits repeat from run to run, and a member's bits depend on its own rows of the arguments
// alone (not on S, not on the other members).  A member whose done[s] != 0 is skipped by all three launches.
// rpo_logreg_step_sets: one workgroup per member, accelerated gradient descent with a fixed step and gradient restart.
#include "common.h"

namespace {

constexpr int LG_ROWS = 32, LG_PAD = 4, LG_WAVES = 8;
constexpr int LG_MAX_E = 1024, LG_MAX_C = 1024, LG_MAX_S = 1024;
constexpr int LG_CHUNK = 1024;                 // rows per gradient partial: fixed, so a member's bits do not depend on S
constexpr int LG_GW = 4;                       // waves (class tiles) per workgroup of the gradient launch
constexpr int LG_STEP_THREADS = 1024;

// acc[r] of v_mfma_f32_32x32x2_f32 is D[(r & 3) + 8 (r >> 2) + 4 half][l31] (lp_head.hip, rpo_probe_mfma)
__device__ __forceinline__ int lg_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__host__ __device__ __forceinline__ int64_t lg_up4(int64_t v) { return (v + 3) & ~(int64_t)3; }

// The workspace: [R (S n C) | part (S chunks C e) | bpart (S chunks C) | lpart (S tiles) | wreg (S) | a (S n)], every
// section starting on a multiple of 4 floats.
struct LgLayout {
  int64_t r, part, bpart, lpart, wreg, a, total;
  int tiles, chunks;
};
__host__ __device__ __forceinline__ LgLayout lg_layout(int n, int C, int e, int S) {
  LgLayout w;
  w.tiles = (n + LG_ROWS - 1) / LG_ROWS;
  w.chunks = (n + LG_CHUNK - 1) / LG_CHUNK;
  w.r = 0;
  w.part = w.r + lg_up4((int64_t)S * n * C);
  w.bpart = w.part + lg_up4((int64_t)S * w.chunks * C * e);
  w.lpart = w.bpart + lg_up4((int64_t)S * w.chunks * C);
  w.wreg = w.lpart + lg_up4((int64_t)S * w.tiles);
  w.a = w.wreg + lg_up4(S);
  w.total = w.a + lg_up4((int64_t)S * n);
  return w;
}

template <int EMAX>
__global__ __launch_bounds__(64 * LG_WAVES) void lg_fwd_kernel(
    const float* __restrict__ feat, int64_t ldf, const int64_t* __restrict__ label, const float* __restrict__ weight,
    const double* __restrict__ omega, const float* __restrict__ l2, const float* __restrict__ params, int64_t ps,
    const int32_t* __restrict__ done, int norm_feat, float* R, float* lpart, float* wreg, float* a_out, int n, int C, int e) {
  __shared__ __attribute__((aligned(16))) float s_feat[LG_ROWS * (EMAX + LG_PAD)];
  __shared__ float s_a[LG_ROWS];
  __shared__ double s_loss[LG_ROWS];
  __shared__ double s_wsq[LG_MAX_C];
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, half = lane >> 5, wv = tid >> 6, nw = blockDim.x >> 6;
  const int i0 = blockIdx.x * LG_ROWS, s = blockIdx.y;
  if (done && done[s]) return;
  const int rows = min(LG_ROWS, n - i0);
  const int ld = e + LG_PAD;
  const float* W = params + (int64_t)s * ps;
  const float* bias = W + (int64_t)C * e;
  float* Rs = R + ((int64_t)s * n + i0) * C;                       // this tile's rows of R

  // ---- stage the rows (rows past n: zeros; their results are never written)
  if ((ldf & 3) == 0) {
    const int q4 = e >> 2;
    for (int idx = tid; idx < LG_ROWS * q4; idx += blockDim.x) {
      const int r = idx / q4, q = idx - r * q4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < rows) v = *reinterpret_cast<const float4*>(feat + (int64_t)(i0 + r) * ldf + 4 * q);
      *reinterpret_cast<float4*>(s_feat + r * ld + 4 * q) = v;
    }
  } else {
    for (int idx = tid; idx < LG_ROWS * e; idx += blockDim.x) {
      const int r = idx / e, k = idx - r * e;
      s_feat[r * ld + k] = r < rows ? feat[(int64_t)(i0 + r) * ldf + k] : 0.f;
    }
  }
  __syncthreads();

  // ---- a_i exactly as rpo_features_classify forms it at scale 1: lane j sums elements j, j + 64, ... in double, a butterfly
  for (int r = wv; r < LG_ROWS; r += nw) {
    float a = 1.0f;
    if (norm_feat) {
      double acc = 0.0;
      for (int k = lane; k < e; k += 64) {
        const double v = (double)s_feat[r * ld + k];
        acc = fma(v, v, acc);
      }
      acc = wave_sum_f64(acc);
      a = (float)(1.0 / sqrt(acc));
    }
    if (lane == 0) {
      s_a[r] = a;
      if (r < rows) a_out[(int64_t)s * n + i0 + r] = a;
    }
  }
  __syncthreads();

  // ---- the logits of this wave's class tiles -> R (as z, for now)
  const bool want_sq = blockIdx.x == 0;
  const int ctiles = (C + 31) >> 5;
  const float* arow = s_feat + l31 * ld + 4 * half;
  for (int ct = wv; ct < ctiles; ct += nw) {
    const int c = ct * 32 + l31;
    const bool cok = c < C;
    const int cc = min(c, C - 1);                                  // (a column past C reads the last row; never kept)
    const float* crow = W + (int64_t)cc * e + 4 * half;
    f32x16_t d;
#pragma unroll
    for (int r = 0; r < 16; ++r) d[r] = 0.f;
    double q = 0.0;
    float4 bv = *reinterpret_cast<const float4*>(crow);
    for (int k = 0; k < e; k += 8) {                               // lane half h holds k .. k+7's elements 4h .. 4h+3
      const float4 av = *reinterpret_cast<const float4*>(arow + k);
      float4 bn = bv;
      if (k + 8 < e) bn = *reinterpret_cast<const float4*>(crow + k + 8);
      if (want_sq) {
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
    if (want_sq) {
      q += __shfl_xor(q, 32, 64);                                  // the two halves of the row: a + b in both lanes
      if (cok && half == 0) s_wsq[c] = q;
    }
    const float bj = bias[cc];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = lg_row(r, half);
      if (cok && row < rows) Rs[(int64_t)row * C + c] = __fmaf_rn(d[r], s_a[row], bj);
    }
  }
  __syncthreads();                                                 // the tile's logits are visible to the whole workgroup

  // ---- softmax, residual and loss: one wave per row, lane l holds classes l, l + 64, ...
  const double om = omega[s];
  for (int r = wv; r < LG_ROWS; r += nw) {
    double lrow = 0.0;
    if (r < rows) {                                                // (wave-uniform)
      float* zr = Rs + (int64_t)r * C;
      float z[LG_MAX_C / 64];
      float m = -INFINITY;
#pragma unroll
      for (int j = 0; j < LG_MAX_C / 64; ++j) {
        const int c = lane + 64 * j;
        z[j] = c < C ? zr[c] : -INFINITY;
        m = fmaxf(m, z[j]);
      }
      m = wave_max(m);
      double se = 0.0;
      float ex[LG_MAX_C / 64];
#pragma unroll
      for (int j = 0; j < LG_MAX_C / 64; ++j) {
        ex[j] = lane + 64 * j < C ? expf(z[j] - m) : 0.f;
        se += (double)ex[j];
      }
      se = wave_sum_f64(se);
      const int64_t lb64 = label[i0 + r];
      const bool ok = lb64 >= 0 && lb64 < C;                       // outside [0, C): weight 0, nothing read
      const int lb = ok ? (int)lb64 : -1;
      const float wt = weight ? weight[(int64_t)s * n + i0 + r] : 1.0f;
      const double cw = ok ? (double)wt / om : 0.0;
      const double inv = 1.0 / se;
      float zl = -INFINITY;
#pragma unroll
      for (int j = 0; j < LG_MAX_C / 64; ++j) {
        const int c = lane + 64 * j;
        if (c == lb) zl = z[j];
        if (c < C) zr[c] = (float)(cw * ((double)ex[j] * inv - (c == lb ? 1.0 : 0.0)));
      }
      zl = wave_max(zl);                                           // the one lane that holds z[label]
      if (ok && wt != 0.f) lrow = cw * (((double)m + log(se)) - (double)zl);
    }
    if (lane == 0) s_loss[r] = lrow;
  }
  __syncthreads();
  if (tid == 0) {
    double acc = 0.0;
    for (int r = 0; r < LG_ROWS; ++r) acc += s_loss[r];
    lpart[(int64_t)s * gridDim.x + blockIdx.x] = (float)acc;
  }
  if (want_sq && wv == 0) {                                        // (l2/2) |W_s|^2: lane l sums classes l, l + 64, ...
    double acc = 0.0;
    for (int c = lane; c < C; c += 64) acc += s_wsq[c];
    acc = wave_sum_f64(acc);
    if (lane == 0) wreg[s] = (float)(0.5 * (double)l2[s] * acc);
  }
}

// G partial of (32 classes, 32 NB features, chunk): D[class][feature] = sum_i R[i][class] (a_i F[i][feature]), i ascending
template <int NB>
__global__ __launch_bounds__(64 * LG_GW) void lg_grad_kernel(const float* __restrict__ feat, int64_t ldf,
                                                             const float* __restrict__ R, const float* __restrict__ a_in,
                                                             const int32_t* __restrict__ done, float* part, float* bpart,
                                                             int n, int C, int e, int chunks) {
  const int lane = threadIdx.x & 63, l31 = lane & 31, half = lane >> 5, wv = threadIdx.x >> 6;
  const int s = blockIdx.z / chunks, ch = blockIdx.z - s * chunks;
  if (done && done[s]) return;
  const int ct = blockIdx.y * LG_GW + wv;
  if (ct * 32 >= C) return;                                        // (no barrier in this kernel)
  const int c = ct * 32 + l31;
  const bool cok = c < C;
  const int cc = min(c, C - 1);
  const int e0 = blockIdx.x * 32 * NB;
  const int r0 = ch * LG_CHUNK, r1 = min(n, r0 + LG_CHUNK);
  const float* Rc = R + (int64_t)s * n * C + cc;
  const float* as = a_in + (int64_t)s * n;
  const float* fc = feat + e0 + l31;
  f32x16_t d[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) d[b][r] = 0.f;
  float bsum = 0.f;
  for (int i = r0; i < r1; i += 8) {                               // four k steps' operands fetched ahead of their MFMAs
    float rv[4], fv[4][NB];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int ii = i + 2 * u + half;
      const bool ok = ii < r1;
      const int ir = ok ? ii : r0;                                 // (a row past the chunk: a valid address, a zero operand)
      rv[u] = ok ? Rc[(int64_t)ir * C] : 0.f;
      const float av = as[ir];
      const float* fr = fc + (int64_t)ir * ldf;
#pragma unroll
      for (int b = 0; b < NB; ++b) fv[u][b] = ok ? fr[32 * b] * av : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      bsum += rv[u];
#pragma unroll
      for (int b = 0; b < NB; ++b) d[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(rv[u], fv[u][b], d[b], 0, 0, 0);
    }
  }
  float* po = part + (((int64_t)s * chunks + ch) * C) * e + e0 + l31;
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = ct * 32 + lg_row(r, half);
      if (row < C) po[(int64_t)row * e + 32 * b] = d[b][r];
    }
  bsum += __shfl_xor(bsum, 32, 64);                                // even rows + odd rows, the same sum in both halves
  if (blockIdx.x == 0 && half == 0 && cok) bpart[((int64_t)s * chunks + ch) * C + c] = bsum;
}

__global__ __launch_bounds__(256) void lg_final_kernel(const float* __restrict__ params, int64_t ps,
                                                       const float* __restrict__ l2, const int32_t* __restrict__ done,
                                                       const float* __restrict__ part, const float* __restrict__ bpart,
                                                       const float* __restrict__ lpart, const float* __restrict__ wreg,
                                                       int fit_bias, float* grads, float* loss, int C, int e, int chunks,
                                                       int tiles) {
  const int c = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
  if (done && done[s]) return;
  const float lam = l2[s];
  const float* W = params + (int64_t)s * ps;
  float* G = grads + (int64_t)s * ps;
  if (tid < (e >> 2)) {
    const float* p = part + ((int64_t)s * chunks * C + c) * e + 4 * tid;
    float4 acc = *reinterpret_cast<const float4*>(p);
    for (int ch = 1; ch < chunks; ++ch) {
      const float4 v = *reinterpret_cast<const float4*>(p + (int64_t)ch * C * e);
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    const float4 w = *reinterpret_cast<const float4*>(W + (int64_t)c * e + 4 * tid);
    *reinterpret_cast<float4*>(G + (int64_t)c * e + 4 * tid) =
        make_float4(__fmaf_rn(lam, w.x, acc.x), __fmaf_rn(lam, w.y, acc.y), __fmaf_rn(lam, w.z, acc.z),
                    __fmaf_rn(lam, w.w, acc.w));
  }
  if (tid == 255) {
    float acc = 0.f;
    if (fit_bias) {
      const float* p = bpart + (int64_t)s * chunks * C + c;
      acc = p[0];
      for (int ch = 1; ch < chunks; ++ch) acc += p[(int64_t)ch * C];
    }
    G[(int64_t)C * e + c] = acc;
  }
  if (c == 0 && tid >= 64 && tid < 128) {                          // the loss: lane l sums tiles l, l + 64, ... in double
    const int lane = tid - 64;
    double acc = 0.0;
    for (int t = lane; t < tiles; t += 64) acc += (double)lpart[(int64_t)s * tiles + t];
    acc = wave_sum_f64(acc);
    if (lane == 0) loss[s] = (float)(acc + (double)wreg[s]);
  }
}

template <int EMAX>
void lg_fwd_launch(dim3 grid, int waves, hipStream_t st, const float* feat, int64_t ldf, const int64_t* label,
                   const float* weight, const double* omega, const float* l2, const float* params, int64_t ps,
                   const int32_t* done, int norm_feat, float* R, float* lpart, float* wreg, float* a_out, int n, int C,
                   int e) {
  hipLaunchKernelGGL((lg_fwd_kernel<EMAX>), grid, dim3(64 * waves), 0, st, feat, ldf, label, weight, omega, l2, params, ps,
                     done, norm_feat, R, lpart, wreg, a_out, n, C, e);
}

template <int NB>
void lg_grad_launch(hipStream_t st, const float* feat, int64_t ldf, const float* R, const float* a_in, const int32_t* done,
                    float* part, float* bpart, int n, int C, int e, int chunks, int S) {
  const dim3 grid(e / (32 * NB), ((C + 31) / 32 + LG_GW - 1) / LG_GW, S * chunks);
  hipLaunchKernelGGL((lg_grad_kernel<NB>), grid, dim3(64 * LG_GW), 0, st, feat, ldf, R, a_in, done, part, bpart, n, C, e,
                     chunks);
}

// x+ = y - g / L; restart (t <- 1) when <g, x+ - x> > 0; t+ = (1 + sqrt(1 + 4 t^2)) / 2; y+ = x+ + ((t - 1) / t+)(x+ - x).
// Pass 1 reduces the restart product (double) and |g|_inf in a fixed order, pass 2 writes.
__global__ __launch_bounds__(LG_STEP_THREADS) void lg_step_kernel(float* x, float* y, const float* __restrict__ g,
                                                                 int64_t ps, int64_t count, float* t,
                                                                 const float* __restrict__ L, const float* __restrict__ tol,
                                                                 int32_t* done, int32_t* iters, float* grad_inf) {
  __shared__ double s_ip[LG_STEP_THREADS / 64];
  __shared__ float s_mx[LG_STEP_THREADS / 64];
  __shared__ int s_nan[LG_STEP_THREADS / 64];
  __shared__ float s_beta;
  __shared__ int s_stop;
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (done[s]) return;                                             // (uniform: one workgroup per member)
  x += (int64_t)s * ps; y += (int64_t)s * ps; g += (int64_t)s * ps;
  const float invL = 1.0f / L[s];
  double ip = 0.0;
  float mx = 0.f;
  int nan = 0;
  for (int64_t j = tid; j < count; j += LG_STEP_THREADS) {
    const float gj = g[j];
    const float xn = __fmaf_rn(-gj, invL, y[j]);
    ip = fma((double)gj, (double)(xn - x[j]), ip);
    const float aj = fabsf(gj);
    mx = aj > mx ? aj : mx;
    nan |= aj != aj;
  }
  ip = wave_sum_f64(ip);
  mx = wave_max(mx);
  nan = __any(nan);
  if (lane == 0) { s_ip[wv] = ip; s_mx[wv] = mx; s_nan[wv] = nan; }
  __syncthreads();
  if (tid == 0) {
    double tip = 0.0;
    float tmx = 0.f;
    int tnan = 0;
    for (int w = 0; w < LG_STEP_THREADS / 64; ++w) { tip += s_ip[w]; tmx = fmaxf(tmx, s_mx[w]); tnan |= s_nan[w]; }
    if (tnan) tmx = __builtin_nanf("");
    grad_inf[s] = tmx;
    const int stop = tmx <= tol[s];
    s_stop = stop;
    if (stop) {
      done[s] = 1;                                                 // the point kept is y: the one whose gradient was tested
    } else {
      const float t0 = tip > 0.0 ? 1.0f : t[s];
      const float t1 = 0.5f * (1.0f + sqrtf(__fmaf_rn(4.0f * t0, t0, 1.0f)));
      s_beta = (t0 - 1.0f) / t1;
      t[s] = t1;
      iters[s] += 1;
    }
  }
  __syncthreads();
  if (s_stop) return;
  const float beta = s_beta;
  for (int64_t j = tid; j < count; j += LG_STEP_THREADS) {
    const float xn = __fmaf_rn(-g[j], invL, y[j]);
    y[j] = __fmaf_rn(beta, xn - x[j], xn);
    x[j] = xn;
  }
}

}  // namespace

extern "C" int64_t rpo_logreg_workspace_floats(int n, int C, int e, int S) {
  if (n <= 0 || C <= 0 || e <= 0 || S <= 0) return 0;
  return lg_layout(n, C, e, S).total;
}

extern "C" int rpo_logreg_loss_grad_sets(const float* feat, int64_t ldf, const int64_t* label, const float* weight,
                                         const double* omega, const float* l2, const float* params, int64_t set_stride,
                                         const int32_t* done, int norm_feat, int fit_bias, float* grads, float* loss, int n,
                                         int C, int e, int S, float* workspace, void* stream) {
  if (!feat || !label || !omega || !l2 || !params || !grads || !loss || !workspace || ldf <= 0 || set_stride <= 0)
    return RPO_E_BADARG;
  if (n < 1 || C < 1 || C > LG_MAX_C || S < 1 || S > LG_MAX_S || e < 32 || e > LG_MAX_E || e % 32 != 0 || ldf < e ||
      set_stride < (int64_t)C * e + C)
    return RPO_E_SHAPE;
  if ((int64_t)S * ((n + LG_CHUNK - 1) / LG_CHUNK) > 65535) return RPO_E_SHAPE;     // (grid.z of the gradient launch)
  if (!aligned16(feat) || !aligned16(params) || !aligned16(grads) || !aligned16(workspace) || set_stride % 4 != 0 ||
      reinterpret_cast<uintptr_t>(omega) % 8)
    return RPO_E_ALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const LgLayout w = lg_layout(n, C, e, S);
  float* R = workspace + w.r;
  float* part = workspace + w.part;
  float* bpart = workspace + w.bpart;
  float* lpart = workspace + w.lpart;
  float* wreg = workspace + w.wreg;
  float* a = workspace + w.a;
  const int ctiles = (C + 31) / 32;
  int waves = 1;                                                                 // every wave has a class tile
  while (2 * waves <= LG_WAVES && 2 * waves <= ctiles) waves *= 2;
  const dim3 grid(w.tiles, S);
  if (e <= 256)
    lg_fwd_launch<256>(grid, waves, st, feat, ldf, label, weight, omega, l2, params, set_stride, done, norm_feat, R, lpart, wreg, a, n, C, e);
  else if (e <= 512)
    lg_fwd_launch<512>(grid, waves, st, feat, ldf, label, weight, omega, l2, params, set_stride, done, norm_feat, R, lpart, wreg, a, n, C, e);
  else
    lg_fwd_launch<1024>(grid, waves, st, feat, ldf, label, weight, omega, l2, params, set_stride, done, norm_feat, R, lpart, wreg, a, n, C, e);
  if (e % 128 == 0)
    lg_grad_launch<4>(st, feat, ldf, R, a, done, part, bpart, n, C, e, w.chunks, S);
  else if (e % 64 == 0)
    lg_grad_launch<2>(st, feat, ldf, R, a, done, part, bpart, n, C, e, w.chunks, S);
  else
    lg_grad_launch<1>(st, feat, ldf, R, a, done, part, bpart, n, C, e, w.chunks, S);
  hipLaunchKernelGGL(lg_final_kernel, dim3(C, S), dim3(256), 0, st, params, set_stride, l2, done, part, bpart, lpart, wreg,
                     fit_bias, grads, loss, C, e, w.chunks, w.tiles);
  return rpo_launch_status();
}

extern "C" int rpo_logreg_step_sets(float* x, float* y, const float* grads, int64_t set_stride, int64_t count, float* t,
                                    const float* L, const float* tol, int32_t* done, int32_t* iters, float* grad_inf, int S,
                                    void* stream) {
  if (!x || !y || !grads || !t || !L || !tol || !done || !iters || !grad_inf || set_stride <= 0) return RPO_E_BADARG;
  if (S < 1 || S > LG_MAX_S || count < 1 || count > set_stride || count > (int64_t)LG_MAX_C * (LG_MAX_E + 1))
    return RPO_E_SHAPE;
  hipLaunchKernelGGL(lg_step_kernel, dim3(S), dim3(LG_STEP_THREADS), 0, static_cast<hipStream_t>(stream), x, y, grads,
                     set_stride, count, t, L, tol, done, iters, grad_inf);
  return rpo_launch_status();
}
