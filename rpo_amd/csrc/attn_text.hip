// Text-tower attention against per-class cached keys/values.
//
// Reference semantics: nn.MultiheadAttention with the per-class additive mask of
// trainers/rpo.py:144-151 (causal AND column < len_c).  The K prompt rows sit at positions
// len_c .. len_c+K-1 (:176-177), i.e. behind every allowed column, so each of them reads
// exactly keys [0, len_c) of its class; frozen token t reads keys [0, min(t+1, len_c)).
//
// Sizes are tiny (<= 77 keys, head_dim 64 = one wave): this is a VALU kernel.  One workgroup
// per (class, head) stages that class's K and V head slices in LDS once; each wave then
// walks query rows.  head_dim 64 == wave size, so "lane = key" for the score / dP passes
// and "lane = feature" for the P.V / dS.K passes; operands are broadcast with v_readlane.
#include "common.h"

namespace {

__device__ __forceinline__ float bcast(float v, int lane_uniform) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane_uniform));
}

// ---- one query row of a wave ------------------------------------------------------------------------------------------
// The lane holds keys `lane` and `lane + 64` (at most 128 keys): k0 / k1 point at their fp32 rows in LDS.
__device__ __forceinline__ void row_dots(float av, const float* k0, const float* k1, float& s0, float& s1) {
  s0 = 0.f; s1 = 0.f;
#pragma unroll 8
  for (int d = 0; d < 64; ++d) {
    const float ad = bcast(av, d);
    s0 = fmaf(ad, k0[d], s0);
    s1 = fmaf(ad, k1[d], s1);
  }
}

// raw scores of keys lane / lane + 64 -> softmax probabilities over the keys [0, nk)
__device__ __forceinline__ void row_softmax(float& s0, float& s1, int nk, float scale, int lane) {
  s0 = lane < nk ? s0 * scale : -INFINITY;
  s1 = lane + 64 < nk ? s1 * scale : -INFINITY;
  const float m = wave_max(fmaxf(s0, s1));
  s0 = expf(s0 - m); s1 = expf(s1 - m);
  const float inv = 1.0f / wave_sum(s0 + s1);
  s0 *= inv; s1 *= inv;
}

// dp_j = <dO, v_j> of keys lane / lane + 64 -> ds_j = p_j (dp_j - sum_j p_j dp_j)
__device__ __forceinline__ void row_ds(float p0, float p1, float& dp0, float& dp1, int nk, int lane) {
  dp0 = lane < nk ? dp0 : 0.f;
  dp1 = lane + 64 < nk ? dp1 : 0.f;
  // an explicit fma: which of the two products `p0 * dp0 + p1 * dp1` contracts into one is the compiler's choice and
  // changes with the code around it; this is the rounding every caller has always had
  const float delta = wave_sum(fmaf(p0, dp0, p1 * dp1));
  dp0 = p0 * (dp0 - delta); dp1 = p1 * (dp1 - delta);
}

// acc + sum over keys j in [j_lo, j_hi), ascending, of w_j * rows[j - j_base][lane] (lane = feature; w0 / w1 hold w_j of
// keys lane / lane + 64)
__device__ __forceinline__ float row_accumulate(float acc, float w0, float w1, int j_lo, int j_hi, const float* rows,
                                                int j_base, int lane) {
  for (int j = j_lo; j < j_hi; ++j) {
    const float wj = j < 64 ? bcast(w0, j) : bcast(w1, j - 64);
    acc = fmaf(wj, rows[(j - j_base) * 65 + lane], acc);
  }
  return acc;
}

// one 16-byte chunk of T (8 or 4 elements) -> fp32 at dst
template <typename T>
__device__ __forceinline__ void unpack_chunk(const uint4& c, float* dst) {
  const uint32_t w[4] = {c.x, c.y, c.z, c.w};
  if constexpr (sizeof(T) == 2) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      dst[2 * e] = unpack1<T>((uint16_t)(w[e] & 0xffffu));
      dst[2 * e + 1] = unpack1<T>((uint16_t)(w[e] >> 16));
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) dst[e] = __uint_as_float(w[e]);
  }
}

template <typename T, bool BWD>
__global__ __launch_bounds__(256) void text_attn_kernel(const T* __restrict__ q, int64_t ldq,
                                                        const T* __restrict__ kc, const T* __restrict__ vc,
                                                        int64_t ldkv, const T* __restrict__ da, int64_t ldda,
                                                        T* out, int64_t ldo, const int32_t* __restrict__ len,
                                                        int rows, int Lmax, int H, int causal, float scale,
                                                        int n_kv) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* Kf = reinterpret_cast<float*>(smem);
  float* Vf = Kf + Lmax * 65;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = blockIdx.x / H, h = blockIdx.x % H;
  const int ckv = c % n_kv;                     // the cached class this (virtual) class reads: c itself when n_kv = n_cls
  const int L = min(len[ckv], Lmax);
  // stage K and V head slices as fp32 [L][65]; 16-B global loads, all issued before the LDS writes
  constexpr int EPC = 16 / sizeof(T);          // elements per 16-B chunk
  constexpr int CPR = 64 / EPC;                // chunks per key row
  constexpr int ITERS = 128 * CPR / 256;       // Lmax <= 128
  uint4 kv[ITERS], vv[ITERS];
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int id = tid + it * 256;
    const int j = id / CPR, cch = id % CPR;
    if (j < L) {
      const int64_t off = ((int64_t)ckv * Lmax + j) * ldkv + h * 64 + cch * EPC;
      kv[it] = *reinterpret_cast<const uint4*>(kc + off);
      vv[it] = *reinterpret_cast<const uint4*>(vc + off);
    }
  }
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int id = tid + it * 256;
    const int j = id / CPR, cch = id % CPR;
    if (j < L) {
      unpack_chunk<T>(kv[it], Kf + j * 65 + cch * EPC);
      unpack_chunk<T>(vv[it], Vf + j * 65 + cch * EPC);
    }
  }
  __syncthreads();
  const int j0 = min(lane, Lmax - 1), j1 = min(lane + 64, Lmax - 1);
  // one query row per wave; blockIdx.y walks the rows in chunks of 4 (each chunk re-stages the tiny K/V
  // slices): a row is ~1.5 k VALU instructions, so spreading rows over workgroups is what shortens the launch
  for (int r = blockIdx.y * 4 + wave; r < rows; r += 4 * gridDim.y) {
    const int64_t row = (int64_t)c * rows + r;
    const int nk = causal ? min(r + 1, L) : L;
    float p0, p1;
    row_dots(ActIO<T>::ld(q + row * ldq + h * 64 + lane), Kf + j0 * 65, Kf + j1 * 65, p0, p1);
    row_softmax(p0, p1, nk, scale, lane);
    if (!BWD) {
      ActIO<T>::st(out + row * ldo + h * 64 + lane, row_accumulate(0.f, p0, p1, 0, nk, Vf, 0, lane));
    } else {
      float ds0, ds1;
      row_dots(ActIO<T>::ld(da + row * ldda + h * 64 + lane), Vf + j0 * 65, Vf + j1 * 65, ds0, ds1);
      row_ds(p0, p1, ds0, ds1, nk, lane);
      ActIO<T>::st(out + row * ldo + h * 64 + lane, row_accumulate(0.f, ds0, ds1, 0, nk, Kf, 0, lane) * scale);
    }
  }
}

// ---- backward of one causal sequence (dQ / dK / dV of all its rows) ---------------------------------------------------
// The sibling trainers train parameters that sit IN FRONT of the class name (CoOp's context vectors, trainers/coop.py:
// 117-134), so their gradient flows through every token of the text tower under the plain causal mask
// (clip/model.py:332-338): autograd of nn.MultiheadAttention for q, k, v of ALL L = len[c] rows of a class.  Rows past
// the EOT token (>= len[c]) cannot reach the text feature (it is read at the EOT row, which sees columns <= itself) and
// get zero gradients.  L <= 80 (CLIP's context is 77), head_dim 64 = one wave:
//   pass 1, one wave per query row r:   p = softmax(scale q_r K^T) over keys j <= r;  dp_j = <dO_r, v_j>;
//           ds_j = p_j (dp_j - sum_j p_j dp_j);   dq_r = scale sum_j ds_j k_j;   P[r][:], DS[r][:] parked in LDS
//   pass 2, one wave per key j:         dk_j = scale sum_{r >= j} DS[r][j] q_r;   dv_j = sum_{r >= j} P[r][j] dO_r
// fp32 arithmetic throughout, fixed summation orders (bit-reproducible).
// A sequence is Pn keys it shares with others (K / V only, rpo_text_attn_bwd_prefix below) followed by Sn rows of its own
// (Q / K / V / dO); Pn = 0, Sn = Lmax is the dense layout of rpo_text_attn_bwd_dense.
struct BwdPrefixLds {                          // floats from the start of the dynamic LDS
  int kp, vp, ak, av, qs, ks, vs, ds, pm, sm, total;
  __host__ __device__ BwdPrefixLds(int Pn, int Sn) {
    kp = 0; vp = kp + Pn * 65; ak = vp + Pn * 65; av = ak + Pn * 64;
    qs = av + Pn * 64; ks = qs + Sn * 65; vs = ks + Sn * 65; ds = vs + Sn * 65;
    pm = ds + Sn * 65; sm = pm + Sn * (Pn + Sn + 1); total = sm + Sn * (Pn + Sn + 1);
  }
};

// The two passes over a staged sequence: Pn shared keys in Kp / Vp and Sn own rows (global rows row0 .., positions Pn ..)
// in Qs / Ks / Vs / Ds, of which the first ns are real and the others zero.  dq of the own rows is written (zeros from ns
// on); dk / dv of the own rows go to the outputs (zeros from ns on) or, unscaled, to own_k / own_v [Sn][64] where those are
// given; the shared keys' share is added to Ak / Av.  Every thread of the workgroup calls it after the barrier that ends
// the staging (one barrier inside).
template <typename T>
__device__ __forceinline__ void bwd_sequence_compute(T* dq, T* dk, T* dv, int64_t ldd, int64_t row0, int col0, int Pn,
                                                     int Sn, int ns, float* lds, const BwdPrefixLds& o, float* own_k,
                                                     float* own_v, float scale, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  const int Lt = Pn + Sn, LP = Lt + 1;
  const float *Kp = lds + o.kp, *Vp = lds + o.vp, *Qs = lds + o.qs, *Ks = lds + o.ks, *Vs = lds + o.vs, *Ds = lds + o.ds;
  float *Ak = lds + o.ak, *Av = lds + o.av, *Pm = lds + o.pm, *Sm = lds + o.sm;
  const int j0 = min(lane, Lt - 1), j1 = min(lane + 64, Lt - 1);
  const float* k0 = j0 < Pn ? Kp + j0 * 65 : Ks + (j0 - Pn) * 65;
  const float* k1 = j1 < Pn ? Kp + j1 * 65 : Ks + (j1 - Pn) * 65;
  const float* v0 = j0 < Pn ? Vp + j0 * 65 : Vs + (j0 - Pn) * 65;
  const float* v1 = j1 < Pn ? Vp + j1 * 65 : Vs + (j1 - Pn) * 65;
  for (int s = wave; s < Sn; s += 4) {
    T* dqr = dq + (row0 + s) * ldd + col0;
    if (s >= ns) {                              // past the EOT: zero gradients (the dX GEMM reads every row)
      ActIO<T>::st(dqr + lane, 0.f);
      continue;
    }
    const int nk = Pn + s + 1;                  // causal, and s < ns: every key up to this row is a real token
    const float qv = Qs[s * 65 + lane], dov = Ds[s * 65 + lane];
    float p0 = 0.f, p1 = 0.f, ds0 = 0.f, ds1 = 0.f;
#pragma unroll 8
    for (int d = 0; d < 64; ++d) {              // row_dots of the scores and of dp in one loop
      const float qd = bcast(qv, d), dd = bcast(dov, d);
      p0 = fmaf(qd, k0[d], p0);
      p1 = fmaf(qd, k1[d], p1);
      ds0 = fmaf(dd, v0[d], ds0);
      ds1 = fmaf(dd, v1[d], ds1);
    }
    row_softmax(p0, p1, nk, scale, lane);
    row_ds(p0, p1, ds0, ds1, nk, lane);
    if (lane < Lt) { Pm[s * LP + lane] = p0; Sm[s * LP + lane] = ds0; }
    if (lane + 64 < Lt) { Pm[s * LP + lane + 64] = p1; Sm[s * LP + lane + 64] = ds1; }
    const float acc = row_accumulate(0.f, ds0, ds1, 0, Pn, Kp, 0, lane);
    ActIO<T>::st(dqr + lane, row_accumulate(acc, ds0, ds1, Pn, nk, Ks, Pn, lane) * scale);
  }
  __syncthreads();
  for (int t = wave; t < Sn; t += 4) {          // the sequence's own keys: read by its rows t .. ns - 1
    float ak = 0.f, av = 0.f;
    for (int s = t; s < ns; ++s) {              // (empty past the EOT: zeros)
      ak = fmaf(Sm[s * LP + Pn + t], Qs[s * 65 + lane], ak);
      av = fmaf(Pm[s * LP + Pn + t], Ds[s * 65 + lane], av);
    }
    if (own_k) {
      own_k[t * 64 + lane] = ak;
      own_v[t * 64 + lane] = av;
    } else {
      ActIO<T>::st(dk + (row0 + t) * ldd + col0 + lane, ak * scale);
      ActIO<T>::st(dv + (row0 + t) * ldd + col0 + lane, av);
    }
  }
  for (int j = wave; j < Pn; j += 4) {          // the shared keys: read by every real row of the sequence
    float ak = Ak[j * 64 + lane], av = Av[j * 64 + lane];
    for (int s = 0; s < ns; ++s) {
      ak = fmaf(Sm[s * LP + j], Qs[s * 65 + lane], ak);
      av = fmaf(Pm[s * LP + j], Ds[s * 65 + lane], av);
    }
    Ak[j * 64 + lane] = ak;
    Av[j * 64 + lane] = av;
  }
}

// rpo_text_attn_bwd_dense: one workgroup per (class, head), the class's Lmax rows as one sequence of no shared keys.  Its
// staging is scalar loads: the entry point has no 16-byte alignment contract (d_out may be any column slice).
template <typename T>
__global__ __launch_bounds__(256) void text_attn_bwd_dense_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                                  const T* __restrict__ v, int64_t ld,
                                                                  const T* __restrict__ dout, int64_t lddo, T* dq, T* dk,
                                                                  T* dv, int64_t ldd, const int32_t* __restrict__ len,
                                                                  int Lmax, int H, float scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* lds = reinterpret_cast<float*>(smem);
  const BwdPrefixLds o(0, Lmax);
  const int tid = threadIdx.x;
  const int c = blockIdx.x / H, h = blockIdx.x % H;
  const int L = min(len[c], Lmax);
  for (int id = tid; id < Lmax * 64; id += 256) {
    const int j = id >> 6, d = id & 63;
    const int64_t row = (int64_t)c * Lmax + j;
    float qv = 0.f, kv = 0.f, vv = 0.f, dv = 0.f;
    if (j < L) {                                // the four loads in flight together, then the LDS writes
      qv = ActIO<T>::ld(q + row * ld + h * 64 + d);
      kv = ActIO<T>::ld(k + row * ld + h * 64 + d);
      vv = ActIO<T>::ld(v + row * ld + h * 64 + d);
      dv = ActIO<T>::ld(dout + row * lddo + h * 64 + d);
    }
    lds[o.qs + j * 65 + d] = qv;
    lds[o.ks + j * 65 + d] = kv;
    lds[o.vs + j * 65 + d] = vv;
    lds[o.ds + j * 65 + d] = dv;
  }
  __syncthreads();
  bwd_sequence_compute<T>(dq, dk, dv, ldd, (int64_t)c * Lmax, h * 64, 0, Lmax, L, lds, o, nullptr, nullptr, scale, tid);
}

template <typename T>
int launch_dense(const void* q, const void* k, const void* v, int64_t ld, const void* dout, int64_t lddo, void* dq,
                 void* dk, void* dv, int64_t ldd, const int32_t* len, int n_cls, int Lmax, int H, float scale,
                 hipStream_t s) {
  static rpo_lds_mask_t lds_ok{0};
  auto kern = text_attn_bwd_dense_kernel<T>;
  const int bytes = BwdPrefixLds(0, Lmax).total * 4;
  if (int rc = rpo_allow_lds(reinterpret_cast<const void*>(kern), BwdPrefixLds(0, 80).total * 4, &lds_ok)) return rc;
  hipLaunchKernelGGL(kern, dim3(n_cls * H), dim3(256), bytes, s, static_cast<const T*>(q), static_cast<const T*>(k),
                     static_cast<const T*>(v), ld, static_cast<const T*>(dout), lddo, static_cast<T*>(dq),
                     static_cast<T*>(dk), static_cast<T*>(dv), ldd, len, Lmax, H, scale);
  return rpo_launch_status();
}

#ifndef RPO_TEXT_ROWS_PER_WG
#define RPO_TEXT_ROWS_PER_WG 4          // query rows per workgroup (one per wave and pass); A/B: tools/build_variant.sh
#endif
template <typename T, bool BWD>
int launch(const void* q, int64_t ldq, const void* kc, const void* vc, int64_t ldkv, const void* da,
           int64_t ldda, void* out, int64_t ldo, const int32_t* len, int n_cls, int rows, int Lmax, int H,
           int causal, float scale, int n_kv, hipStream_t s) {
  static rpo_lds_mask_t lds_ok{0};
  auto kern = text_attn_kernel<T, BWD>;
  const int bytes = 2 * Lmax * 65 * 4;
  if (int rc = rpo_allow_lds(reinterpret_cast<const void*>(kern), 2 * 128 * 65 * 4, &lds_ok)) return rc;
  hipLaunchKernelGGL(kern, dim3(n_cls * H, (rows + RPO_TEXT_ROWS_PER_WG - 1) / RPO_TEXT_ROWS_PER_WG), dim3(256), bytes, s, static_cast<const T*>(q), ldq,
                     static_cast<const T*>(kc), static_cast<const T*>(vc), ldkv, static_cast<const T*>(da), ldda,
                     static_cast<T*>(out), ldo, len, rows, Lmax, H, causal, scale, n_kv);
  return rpo_launch_status();
}

// ---- causal forward with a per-image shared prefix (rpo_text_attn_fwd_prefix) -----------------------------------------
// CoCoOp's prompt of image b and class c is [SOS | ctx + bias[b] | name . EOT] (trainers/cocoop.py:123-161) under the plain
// causal mask: the first P = 1 + n_ctx rows read only themselves, so through every block they are the same for all classes
// of an image and are stored ONCE per image.  Rows: n_img * P prefix rows (b * P + p), then the suffix rows
// n_img * P + (b * n_cls + c) * S + s, which stand for position P + s of sequence (b, c).  One workgroup per (image, head,
// group of PREFIX_GROUP classes) and chunk of PREFIX_ROWS suffix rows (blockIdx.y) stages the image's P prefix keys /
// values once and walks its classes NC at a time: every class in flight has its own S-row suffix region behind the prefix
// (only the keys the chunk's rows can see are staged), wave w serves slot w % NC and the chunk's rows w / NC, w / NC + 4 / NC,
// ...  Four classes x four rows = four rows per wave: a row is ~1.5 k dependent VALU instructions, so, as for
// text_attn_kernel, spreading the rows over workgroups is what shortens a launch (measured with 8 classes x all rows per
// workgroup: one image x 19 classes took 0.7 ms longer per 12-block pass than the dense kernel on MORE rows).  The
// workgroup of class group 0 and row chunk 0 also writes the P prefix rows' outputs.
// Arithmetic: text_attn_kernel's causal forward, operation for operation (lane = key for the scores, keys in position
// order, the same reductions) -- key j is prefix row j below P and suffix row j - P from there on, which changes where an
// operand is read and nothing else: the bits of rpo_text_attn_fwd(causal = 1) on the sequences gathered densely.
constexpr int PREFIX_GROUP = 4;                // classes per workgroup: the P-row prefix is staged once per 4 classes x 4 rows
constexpr int PREFIX_ROWS = 4;                 // suffix rows per class and workgroup

template <typename T>
__device__ __forceinline__ void stage_kv_rows(const T* __restrict__ k, const T* __restrict__ v, int64_t ld, int64_t row0,
                                              int nrows, int col0, float* Kd, float* Vd, int tid) {
  constexpr int EPC = 16 / sizeof(T);          // elements per 16-B chunk
  constexpr int CPR = 64 / EPC;                // chunks per key row
  for (int id = tid; id < nrows * CPR; id += 256) {
    const int j = id / CPR, cch = id % CPR;
    const int64_t off = (row0 + j) * ld + col0 + cch * EPC;
    const uint4 kq = *reinterpret_cast<const uint4*>(k + off);
    const uint4 vq = *reinterpret_cast<const uint4*>(v + off);
    unpack_chunk<T>(kq, Kd + j * 65 + cch * EPC);
    unpack_chunk<T>(vq, Vd + j * 65 + cch * EPC);
  }
}

// one query row of a wave: keys [0, nk), the first min(nk, P) of them in Kp / Vp, the others in Ks / Vs
template <typename T>
__device__ __forceinline__ void prefix_attn_row(const T* __restrict__ qrow, T* orow, const float* Kp, const float* Vp,
                                                const float* Ks, const float* Vs, int P, int Lmax, int nk, float scale,
                                                int lane) {
  const int j0 = min(lane, Lmax - 1), j1 = min(lane + 64, Lmax - 1);
  const float* k0 = j0 < P ? Kp + j0 * 65 : Ks + (j0 - P) * 65;
  const float* k1 = j1 < P ? Kp + j1 * 65 : Ks + (j1 - P) * 65;
  float p0, p1;
  row_dots(ActIO<T>::ld(qrow + lane), k0, k1, p0, p1);
  row_softmax(p0, p1, nk, scale, lane);
  const int np = min(nk, P);
  const float acc = row_accumulate(0.f, p0, p1, 0, np, Vp, 0, lane);
  ActIO<T>::st(orow + lane, row_accumulate(acc, p0, p1, np, nk, Vs, P, lane));
}

template <typename T>
__global__ __launch_bounds__(256) void text_attn_prefix_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                               const T* __restrict__ v, int64_t ld, T* out, int64_t ldo,
                                                               const int32_t* __restrict__ len, int n_img, int n_cls,
                                                               int P, int S, int H, int NC, int groups, float scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* Kp = reinterpret_cast<float*>(smem);   // [P][65]
  float* Vp = Kp + P * 65;
  float* Sb = Vp + P * 65;                      // NC slots of (K [S][65] | V [S][65])
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = blockIdx.x % H, bg = blockIdx.x / H;
  const int g = bg % groups, b = bg / groups;
  const int Lmax = P + S, col0 = h * 64;
  const int64_t suf0 = (int64_t)n_img * P;      // first suffix row
  stage_kv_rows<T>(k, v, ld, (int64_t)b * P, P, col0, Kp, Vp, tid);
  __syncthreads();
  if (g == 0 && blockIdx.y == 0) {              // the image's own prefix rows: row p reads prefix keys 0 .. p
    for (int p = wave; p < P; p += 4) {
      const int64_t row = (int64_t)b * P + p;
      prefix_attn_row<T>(q + row * ld + col0, out + row * ldo + col0, Kp, Vp, Sb, Sb, P, Lmax, p + 1, scale, lane);
    }
  }
  const int c_end = min(n_cls, (g + 1) * PREFIX_GROUP);
  const int s_lo = blockIdx.y * PREFIX_ROWS, s_hi = min(S, s_lo + PREFIX_ROWS);      // this workgroup's suffix rows
  const int slot = wave % NC, s_first = s_lo + wave / NC, s_step = 4 / NC;
  for (int c0 = g * PREFIX_GROUP; c0 < c_end; c0 += NC) {      // (uniform over the workgroup: the barriers below)
    for (int i = 0; i < NC && c0 + i < c_end; ++i) {
      const int L = min(len[c0 + i], Lmax);
      const int ns = max(0, min(s_hi, L - P));   // suffix keys the rows below s_hi of this class read
      float* Ks = Sb + i * 2 * S * 65;
      stage_kv_rows<T>(k, v, ld, suf0 + ((int64_t)b * n_cls + c0 + i) * S, ns, col0, Ks, Ks + S * 65, tid);
    }
    __syncthreads();
    const int c = c0 + slot;
    if (c < c_end) {
      const int L = min(len[c], Lmax);
      const float* Ks = Sb + slot * 2 * S * 65;
      for (int s = s_first; s < s_hi; s += s_step) {
        const int64_t row = suf0 + ((int64_t)b * n_cls + c) * S + s;
        prefix_attn_row<T>(q + row * ld + col0, out + row * ldo + col0, Kp, Vp, Ks, Ks + S * 65, P, Lmax,
                           min(P + s + 1, L), scale, lane);
      }
    }
    __syncthreads();                            // the slots are re-staged by the next round
  }
}

// classes in flight per workgroup: the most of 4, 2, 1 whose LDS stays within 32 KB (five workgroups per CU of 160 KB: the
// rows are chains of dependent VALU and LDS instructions, which other waves hide); one class alone needs at most
// 2 * 80 * 65 * 4 = 41.6 KB
static inline int prefix_lds_bytes(int P, int S, int NC) { return 2 * 65 * 4 * (P + NC * S); }

template <typename T>
int launch_prefix(const void* q, const void* k, const void* v, int64_t ld, void* out, int64_t ldo, const int32_t* len,
                  int n_img, int n_cls, int P, int S, int H, float scale, hipStream_t s) {
  static rpo_lds_mask_t lds_ok{0};
  auto kern = text_attn_prefix_kernel<T>;
  int NC = 4;
  while (NC > 1 && prefix_lds_bytes(P, S, NC) > 32 * 1024) NC >>= 1;
  const int groups = (n_cls + PREFIX_GROUP - 1) / PREFIX_GROUP;
  if (int rc = rpo_allow_lds(reinterpret_cast<const void*>(kern), 64 * 1024, &lds_ok)) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)((int64_t)n_img * groups * H), (S + PREFIX_ROWS - 1) / PREFIX_ROWS), dim3(256),
                     prefix_lds_bytes(P, S, NC), s,
                     static_cast<const T*>(q), static_cast<const T*>(k), static_cast<const T*>(v), ld, static_cast<T*>(out),
                     ldo, len, n_img, n_cls, P, S, H, NC, groups, scale);
  return rpo_launch_status();
}

// ---- backward with a per-image shared prefix (rpo_text_attn_bwd_prefix) ----------------------------------------------
// The backward of text_attn_prefix_kernel's attention, for the trainers whose learned rows ARE the prefix (CoOp's context,
// trainers/coop.py:117-134; CoCoOp's per image, trainers/cocoop.py:123-161): text_attn_bwd_dense_kernel's math on the row
// layout above.  A suffix row is a query and a key of ONE sequence, so its dq / dk / dv are that sequence's; a prefix row is
// a key of every class of its image, so its dk / dv are the prefix's own P x P causal part plus the sum over the classes of
// what their suffix queries contribute -- summed HERE, in every block, which is what lets LayerNorm backward and the dX
// GEMMs (linear in the incoming gradient) run on the one shared row too.
// One workgroup per (image, head, slot).  Slots 0 .. groups - 1 walk `group` classes each: the image's P prefix K / V
// head slices are staged once, then per class its S suffix rows' Q / K / V / dO; the two passes are bwd_sequence_compute's,
// with key j in the prefix arrays below P and in the class's own from there on.
// What the class's queries give prefix key j is accumulated in LDS (Ak / Av [P][64]: element (j, lane) belongs to wave
// j % 4 alone), classes in ascending order, rows in ascending order, and written as an fp32 partial to the workspace.  The
// last slot (`groups`) is the prefix itself: the same routine on a sequence of no shared keys and P own rows, whose dq goes
// to the prefix rows and whose dk / dv go to the workspace.  text_attn_bwd_prefix_reduce then adds, per prefix key, the
// slots in ascending order (class groups, then the self part) and rounds once: no atomics, no arrival order -- the same
// bits every time, and image b's bits do not depend on the other images of the launch (the grouping is a function of
// n_cls and H alone).
// Stages a sequence's Sn own rows (the shared keys are already in Kp / Vp) and runs bwd_sequence_compute on it.  Every
// thread of the workgroup calls it (barriers inside).
template <typename T>
__device__ __forceinline__ void bwd_prefix_sequence(const T* __restrict__ q, const T* __restrict__ k,
                                                    const T* __restrict__ v, int64_t ld, const T* __restrict__ dout,
                                                    int64_t lddo, T* dq, T* dk, T* dv, int64_t ldd, int64_t row0, int col0,
                                                    int Pn, int Sn, int ns, float* lds, const BwdPrefixLds& o,
                                                    float* own_k, float* own_v, float scale, int tid) {
  float *Qs = lds + o.qs, *Ks = lds + o.ks, *Vs = lds + o.vs, *Ds = lds + o.ds;
  stage_kv_rows<T>(k, v, ld, row0, ns, col0, Ks, Vs, tid);
  for (int id = tid; id < Sn * 64; id += 256) {
    const int s = id >> 6, d = id & 63;
    const bool ok = s < ns;
    Qs[s * 65 + d] = ok ? ActIO<T>::ld(q + (row0 + s) * ld + col0 + d) : 0.f;
    Ds[s * 65 + d] = ok ? ActIO<T>::ld(dout + (row0 + s) * lddo + col0 + d) : 0.f;
    if (!ok) { Ks[s * 65 + d] = 0.f; Vs[s * 65 + d] = 0.f; }
  }
  __syncthreads();
  bwd_sequence_compute<T>(dq, dk, dv, ldd, row0, col0, Pn, Sn, ns, lds, o, own_k, own_v, scale, tid);
  __syncthreads();                              // the next sequence re-stages the own rows
}

template <typename T>
__global__ __launch_bounds__(256) void text_attn_bwd_prefix_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                                   const T* __restrict__ v, int64_t ld,
                                                                   const T* __restrict__ dout, int64_t lddo, T* dq, T* dk,
                                                                   T* dv, int64_t ldd, const int32_t* __restrict__ len,
                                                                   int n_img, int n_cls, int P, int S, int H, int group,
                                                                   int groups, float scale, float* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* lds = reinterpret_cast<float*>(smem);
  const int tid = threadIdx.x;
  const int slots = groups + 1;
  const int h = blockIdx.x % H, bg = blockIdx.x / H;
  const int g = bg % slots, b = bg / slots;
  const int col0 = h * 64;
  float* part = ws + (((int64_t)b * H + h) * slots + g) * 2 * P * 64;      // this slot's [dk | dv][P][64] partial
  if (g == groups) {                            // the prefix's own P x P causal attention
    const BwdPrefixLds o(0, P);
    bwd_prefix_sequence<T>(q, k, v, ld, dout, lddo, dq, dk, dv, ldd, (int64_t)b * P, col0, 0, P, P, lds, o, part,
                           part + P * 64, scale, tid);
    return;
  }
  const BwdPrefixLds o(P, S);
  stage_kv_rows<T>(k, v, ld, (int64_t)b * P, P, col0, lds + o.kp, lds + o.vp, tid);
  for (int id = tid; id < 2 * P * 64; id += 256) lds[o.ak + id] = 0.f;      // Ak and Av are adjacent
  // (the first barrier inside bwd_prefix_sequence orders these writes before any read)
  const int c_end = min(n_cls, (g + 1) * group);
  const int64_t suf0 = (int64_t)n_img * P;      // first suffix row
  for (int c = g * group; c < c_end; ++c) {
    const int ns = max(0, min(len[c], P + S) - P);
    bwd_prefix_sequence<T>(q, k, v, ld, dout, lddo, dq, dk, dv, ldd, suf0 + ((int64_t)b * n_cls + c) * S, col0, P, S, ns,
                           lds, o, nullptr, nullptr, scale, tid);
  }
  for (int id = tid; id < 2 * P * 64; id += 256) part[id] = lds[o.ak + id];
}

template <typename T>
__global__ __launch_bounds__(128) void text_attn_bwd_prefix_reduce(const float* __restrict__ ws, T* dk, T* dv, int64_t ldd,
                                                                   int P, int H, int slots, float scale) {
  const int j = blockIdx.x % P, bh = blockIdx.x / P;
  const int h = bh % H, b = bh / H;
  const int which = threadIdx.x >> 6, lane = threadIdx.x & 63;      // wave 0: dk, wave 1: dv
  const float* src = ws + ((int64_t)bh * slots * 2 + which) * P * 64 + j * 64 + lane;
  float acc = 0.f;
  for (int g = 0; g < slots; ++g) acc += src[(int64_t)g * 2 * P * 64];   // class groups in order, the self part last
  const int64_t off = ((int64_t)b * P + j) * ldd + h * 64 + lane;
  if (which) ActIO<T>::st(dv + off, acc);
  else ActIO<T>::st(dk + off, acc * scale);
}

// classes per workgroup: 1 until the (class, head) pairs alone exceed ~1024 workgroups per image (four per CU), then as
// many as keep it there, at most 16 -- a class is S rows of ~1.5 k dependent VALU instructions each, so below that count
// more workgroups shorten the launch and above it a larger group shrinks the workspace.  A function of n_cls and H only.
static inline int bwd_prefix_group(int n_cls, int H) {
  const int64_t g = ((int64_t)n_cls * H + 1023) / 1024;
  return g < 1 ? 1 : g > 16 ? 16 : (int)g;
}
static inline int bwd_prefix_groups(int n_cls, int H) {
  const int group = bwd_prefix_group(n_cls, H);
  return (n_cls + group - 1) / group;
}
static inline int bwd_prefix_lds_floats(int P, int S) {
  const int a = BwdPrefixLds(P, S).total, b = BwdPrefixLds(0, P).total;
  return a > b ? a : b;
}

template <typename T>
int launch_bwd_prefix(const void* q, const void* k, const void* v, int64_t ld, const void* dout, int64_t lddo, void* dq,
                      void* dk, void* dv, int64_t ldd, const int32_t* len, int n_img, int n_cls, int P, int S, int H,
                      float scale, float* ws, hipStream_t s) {
  static rpo_lds_mask_t lds_ok{0};
  auto kern = text_attn_bwd_prefix_kernel<T>;
  const int group = bwd_prefix_group(n_cls, H), groups = bwd_prefix_groups(n_cls, H);
  // the most any P + S <= 80 needs is 33 596 floats (P = 1, S = 79)
  if (int rc = rpo_allow_lds(reinterpret_cast<const void*>(kern), 136 * 1024, &lds_ok)) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)((int64_t)n_img * (groups + 1) * H)), dim3(256), bwd_prefix_lds_floats(P, S) * 4,
                     s, static_cast<const T*>(q), static_cast<const T*>(k), static_cast<const T*>(v), ld,
                     static_cast<const T*>(dout), lddo, static_cast<T*>(dq), static_cast<T*>(dk), static_cast<T*>(dv), ldd,
                     len, n_img, n_cls, P, S, H, group, groups, scale, ws);
  if (int rc = rpo_launch_status()) return rc;
  hipLaunchKernelGGL(text_attn_bwd_prefix_reduce<T>, dim3((unsigned)((int64_t)n_img * H * P)), dim3(128), 0, s, ws,
                     static_cast<T*>(dk), static_cast<T*>(dv), ldd, P, H, groups + 1, scale);
  return rpo_launch_status();
}

// f(T{}) for the storage type T of `dtype`
template <typename F>
int by_dtype(int dtype, F&& f) {
  if (dtype == RPO_F16) return f(f16_t{});
  if (dtype == RPO_BF16) return f(bf16_t{});
  if (dtype == RPO_F32) return f(float{});
  return RPO_E_DTYPE;
}

}  // namespace

// n_kv < n_cls: the n_cls classes are VIRTUAL -- class v reads len[v % n_kv] and the cache rows of class v % n_kv
// (rpo_text_attn_fwd_shared / _bwd_shared: several prompt sets against one cache); n_kv = n_cls is the plain call.
static int text_attn_fwd_impl(const void* q, int64_t ldq, const void* kc, const void* vc, int64_t ldkv, void* out,
                              int64_t ldo, int dtype, const int32_t* len, int n_cls, int n_kv, int rows, int Lmax, int H,
                              int causal, float scale, void* stream) {
  if (!q || !kc || !vc || !out || !len || n_cls <= 0 || rows <= 0 || Lmax <= 0 || H <= 0) return RPO_E_BADARG;
  if (Lmax > 128) return RPO_E_SHAPE;
  {
    const int esz = dtype == RPO_F32 ? 4 : 2;
    if (!aligned16(kc) || !aligned16(vc) || (ldkv * esz) % 16 != 0) return RPO_E_ALIGN;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
#ifndef RPO_TEXT_ATTN_VALU
  if (!causal) {
    const int rc = rpo_text_attn_wave(0, q, ldq, kc, vc, ldkv, nullptr, 0, out, ldo, dtype, len, n_cls, n_kv, rows, Lmax, H, scale, s);
    if (rc != RPO_E_SHAPE) return rc;
  }
#endif
  return by_dtype(dtype, [&](auto t) {
    return launch<decltype(t), false>(q, ldq, kc, vc, ldkv, nullptr, 0, out, ldo, len, n_cls, rows, Lmax, H, causal, scale,
                                      n_kv, s);
  });
}

static int text_attn_bwd_impl(const void* q, int64_t ldq, const void* kc, const void* vc, int64_t ldkv, const void* da,
                              int64_t ldda, void* dq, int64_t lddq, int dtype, const int32_t* len, int n_cls, int n_kv,
                              int rows, int Lmax, int H, float scale, void* stream) {
  if (!q || !kc || !vc || !da || !dq || !len || n_cls <= 0 || rows <= 0 || Lmax <= 0 || H <= 0) return RPO_E_BADARG;
  if (Lmax > 128) return RPO_E_SHAPE;
  {
    const int esz = dtype == RPO_F32 ? 4 : 2;
    if (!aligned16(kc) || !aligned16(vc) || (ldkv * esz) % 16 != 0) return RPO_E_ALIGN;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
#ifndef RPO_TEXT_ATTN_VALU
  {
    const int rc = rpo_text_attn_wave(1, q, ldq, kc, vc, ldkv, da, ldda, dq, lddq, dtype, len, n_cls, n_kv, rows, Lmax, H, scale, s);
    if (rc != RPO_E_SHAPE) return rc;
  }
#endif
  return by_dtype(dtype, [&](auto t) {
    return launch<decltype(t), true>(q, ldq, kc, vc, ldkv, da, ldda, dq, lddq, len, n_cls, rows, Lmax, H, 0, scale, n_kv, s);
  });
}

extern "C" int rpo_text_attn_fwd(const void* q, int64_t ldq, const void* kc, const void* vc, int64_t ldkv,
                                 void* out, int64_t ldo, int dtype, const int32_t* len, int n_cls, int rows,
                                 int Lmax, int H, int causal, float scale, void* stream) {
  return text_attn_fwd_impl(q, ldq, kc, vc, ldkv, out, ldo, dtype, len, n_cls, n_cls, rows, Lmax, H, causal, scale, stream);
}

extern "C" int rpo_text_attn_bwd(const void* q, int64_t ldq, const void* kc, const void* vc, int64_t ldkv,
                                 const void* da, int64_t ldda, void* dq, int64_t lddq, int dtype,
                                 const int32_t* len, int n_cls, int rows, int Lmax, int H, float scale,
                                 void* stream) {
  return text_attn_bwd_impl(q, ldq, kc, vc, ldkv, da, ldda, dq, lddq, dtype, len, n_cls, n_cls, rows, Lmax, H, scale, stream);
}

extern "C" int rpo_text_attn_fwd_shared(const void* q, int64_t ldq, const void* kc, const void* vc, int64_t ldkv,
                                        void* out, int64_t ldo, int dtype, const int32_t* len, int n_cls, int n_kv,
                                        int rows, int Lmax, int H, float scale, void* stream) {
  if (n_kv <= 0) return RPO_E_BADARG;
  if (n_cls % n_kv != 0) return RPO_E_SHAPE;
  return text_attn_fwd_impl(q, ldq, kc, vc, ldkv, out, ldo, dtype, len, n_cls, n_kv, rows, Lmax, H, 0, scale, stream);
}

extern "C" int rpo_text_attn_bwd_shared(const void* q, int64_t ldq, const void* kc, const void* vc, int64_t ldkv,
                                        const void* da, int64_t ldda, void* dq, int64_t lddq, int dtype,
                                        const int32_t* len, int n_cls, int n_kv, int rows, int Lmax, int H, float scale,
                                        void* stream) {
  if (n_kv <= 0) return RPO_E_BADARG;
  if (n_cls % n_kv != 0) return RPO_E_SHAPE;
  return text_attn_bwd_impl(q, ldq, kc, vc, ldkv, da, ldda, dq, lddq, dtype, len, n_cls, n_kv, rows, Lmax, H, scale, stream);
}

extern "C" int rpo_text_attn_bwd_dense(const void* q, const void* k, const void* v, int64_t ld, const void* d_out,
                                       int64_t lddo, void* dq, void* dk, void* dv, int64_t ldd, int dtype,
                                       const int32_t* len, int n_cls, int Lmax, int H, float scale, void* stream) {
  if (!q || !k || !v || !d_out || !dq || !dk || !dv || !len || n_cls <= 0 || Lmax <= 0 || H <= 0) return RPO_E_BADARG;
  if (Lmax > 80) return RPO_E_SHAPE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return by_dtype(dtype, [&](auto t) {
    return launch_dense<decltype(t)>(q, k, v, ld, d_out, lddo, dq, dk, dv, ldd, len, n_cls, Lmax, H, scale, s);
  });
}

extern "C" int rpo_text_attn_fwd_prefix(const void* q, const void* k, const void* v, int64_t ld, void* out, int64_t ldo,
                                        int dtype, const int32_t* len, int n_img, int n_cls, int P, int S, int H,
                                        float scale, void* stream) {
  if (!q || !k || !v || !out || !len || n_img < 1 || n_cls < 1 || P < 1 || S < 1 || H < 1) return RPO_E_BADARG;
  if ((int64_t)P + S > 80) return RPO_E_SHAPE;
  const int64_t wgs = (int64_t)n_img * ((n_cls + PREFIX_GROUP - 1) / PREFIX_GROUP) * H;
  if (wgs > 2147483647ll) return RPO_E_SHAPE;
  if (dtype != RPO_F32 && dtype != RPO_BF16 && dtype != RPO_F16) return RPO_E_DTYPE;
  const int esz = dtype == RPO_F32 ? 4 : 2;
  if (!aligned16(k) || !aligned16(v) || (ld * esz) % 16 != 0 || (ldo * esz) % 16 != 0) return RPO_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return by_dtype(dtype, [&](auto t) {
    return launch_prefix<decltype(t)>(q, k, v, ld, out, ldo, len, n_img, n_cls, P, S, H, scale, s);
  });
}

extern "C" int64_t rpo_text_attn_bwd_prefix_workspace_floats(int n_img, int n_cls, int P, int H) {
  if (n_img < 1 || n_cls < 1 || P < 1 || H < 1) return 0;
  return (int64_t)n_img * H * (bwd_prefix_groups(n_cls, H) + 1) * 2 * P * 64;
}

extern "C" int rpo_text_attn_bwd_prefix(const void* q, const void* k, const void* v, int64_t ld, const void* d_out,
                                        int64_t lddo, void* dq, void* dk, void* dv, int64_t ldd, int dtype,
                                        const int32_t* len, int n_img, int n_cls, int P, int S, int H, float scale,
                                        float* workspace, void* stream) {
  if (!q || !k || !v || !d_out || !dq || !dk || !dv || !len || !workspace || n_img < 1 || n_cls < 1 || P < 1 || S < 1 ||
      H < 1)
    return RPO_E_BADARG;
  if ((int64_t)P + S > 80) return RPO_E_SHAPE;
  const int64_t wgs = (int64_t)n_img * (bwd_prefix_groups(n_cls, H) + 1) * H, wgs_reduce = (int64_t)n_img * H * P;
  if (wgs > 2147483647ll || wgs_reduce > 2147483647ll) return RPO_E_SHAPE;
  if (dtype != RPO_F32 && dtype != RPO_BF16 && dtype != RPO_F16) return RPO_E_DTYPE;
  const int esz = dtype == RPO_F32 ? 4 : 2;
  if (!aligned16(k) || !aligned16(v) || !aligned16(workspace) || (ld * esz) % 16 != 0 || (lddo * esz) % 16 != 0 ||
      (ldd * esz) % 16 != 0)
    return RPO_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return by_dtype(dtype, [&](auto t) {
    return launch_bwd_prefix<decltype(t)>(q, k, v, ld, d_out, lddo, dq, dk, dv, ldd, len, n_img, n_cls, P, S, H, scale,
                                          workspace, s);
  });
}
