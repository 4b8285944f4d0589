// The CLIP ResNet image tower (clip/model.py:10-152, ModifiedResNet): NHWC convolutions with the eval-mode BatchNorm
// folded into weight and bias, the anti-aliasing average pools, and the attention pool's two kernels of its own.
//   conv:      y = act(x (*) w + bias [+ resid]), 1x1 / 3x3 (pad 1), stride 1, as an implicit GEMM
//              [B*H*W, taps*Cin] x [Cout, taps*Cin]^T: k is ordered (tap, channel), so every k-slab of 64 bytes of
//              channels belongs to one tap and its A tile is a gather of shifted pixel rows (zero outside the image).
//              No im2col buffer.  2 x 2 waves per workgroup, each a WM x WN grid of 32 x 32 MFMA tiles; the next slab's
//              global loads are in flight while the current one runs from LDS.  16-bit: v_mfma_f32_32x32x16_{bf16,f16};
//              f32: v_mfma_f32_32x32x2_f32.  Every output is summed by one wave in a fixed k order (no atomics).
//   stem:      the first 3x3 stride-2 conv (Cin 3) straight from the fp32 NCHW image, fp32 FMA, one pixel per thread.
//   avgpool:   AvgPool2d(k) (kernel = stride = k) on NHWC rows, fp32 sums in a fixed order.
//   tokens:    attention-pool input: [mean over H*W | the H*W pixels] + positional embedding (clip/model.py:67-69).
//   attnpool:  the one query the pool returns (x[0], :91): per (image, head) an fp32 softmax over the H*W + 1 keys.
#include "common.h"

namespace {

constexpr int CV_ROWB = 80;                    // LDS bytes per tile row: 64 bytes of k plus 16 of padding
constexpr int CV_MAX_T = 256;                  // attention-pool keys (H*W + 1)

template <typename T> struct Vec8;             // 8 consecutive elements <-> fp32
template <> struct Vec8<float> {
  static __device__ __forceinline__ void ld(const float* p, float* v) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  }
  static __device__ __forceinline__ void st(float* p, const float* v) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
  }
};
template <typename T> struct Vec8 {            // bf16_t / f16_t
  static __device__ __forceinline__ void ld(const T* p, float* v) {
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] = unpack1<T>((uint16_t)(w[i] & 0xffffu));
      v[2 * i + 1] = unpack1<T>((uint16_t)(w[i] >> 16));
    }
  }
  static __device__ __forceinline__ void st(T* p, const float* v) {
    *reinterpret_cast<uint4*>(p) = make_uint4(pack2<T>(v[0], v[1]), pack2<T>(v[2], v[3]), pack2<T>(v[4], v[5]),
                                              pack2<T>(v[6], v[7]));
  }
};

// One 32 x 32 x (16 bytes per lane) step: 16-bit = one MFMA over 8 k; f32 = four MFMAs over the lane half's 4 k (A and B
// use the same k permutation, so the product is the same sum in a fixed order).
template <typename T> __device__ __forceinline__ f32x16_t cv_mfma(uint4 a, uint4 b, f32x16_t d) {
  return mfma16<T>(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), d);
}
template <> __device__ __forceinline__ f32x16_t cv_mfma<float>(uint4 a, uint4 b, f32x16_t d) {
  d = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.x), __uint_as_float(b.x), d, 0, 0, 0);
  d = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.y), __uint_as_float(b.y), d, 0, 0, 0);
  d = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.z), __uint_as_float(b.z), d, 0, 0, 0);
  d = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.w), __uint_as_float(b.w), d, 0, 0, 0);
  return d;
}

// y[m][n] = act(sum_k A[m][k] w[n][k] + bias[n] (+ resid[m][n])), m = (b, y, x) pixel, k = (tap, channel).
// 256 threads = 2 x 2 waves; workgroup tile BM x BN = (64 WM) x (64 WN).  Loader: thread t moves 16-byte chunk (t & 3) of
// tile rows (t >> 2) + 64 i.
template <typename T, int WM, int WN>
__global__ __launch_bounds__(256) void conv_kernel(const T* __restrict__ x, const T* __restrict__ w,
                                                   const float* __restrict__ bias, const T* __restrict__ resid, T* y,
                                                   int B, int H, int W, int Cin, int Cout, int ks, int relu) {
  constexpr int BM = 64 * WM, BN = 64 * WN, CK = 64 / (int)sizeof(T);
  __shared__ __attribute__((aligned(16))) unsigned char lds[(BM + BN) * CV_ROWB];
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, half = lane >> 5, wv = tid >> 6;
  const int wm = wv & 1, wn = wv >> 1;
  const int64_t M = (int64_t)B * H * W;
  const int64_t m0 = (int64_t)blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const int chunk = tid & 3, rbase = tid >> 2;
  const int K = ks * ks * Cin, cslabs = Cin / CK, nslab = ks * ks * cslabs, pad = ks >> 1;

  // per loader row: image, pixel coordinates (y = -1 << 20 marks a row past M: every tap lands outside)
  int rb[WM], ry[WM], rx[WM];
#pragma unroll
  for (int i = 0; i < WM; ++i) {
    const int64_t m = m0 + rbase + 64 * i;
    if (m < M) {
      const int64_t hw = (int64_t)H * W;
      rb[i] = (int)(m / hw);
      const int p = (int)(m - (int64_t)rb[i] * hw);
      ry[i] = p / W;
      rx[i] = p - ry[i] * W;
    } else {
      rb[i] = 0; ry[i] = -(1 << 20); rx[i] = 0;
    }
  }
  uint4 ra[WM], rw[WN];
  auto load = [&](int s) {
    const int t = s / cslabs, c0 = (s - t * cslabs) * CK;
    const int dy = t / ks - pad, dx = t - (t / ks) * ks - pad;
#pragma unroll
    for (int i = 0; i < WM; ++i) {
      const int ys = ry[i] + dy, xs = rx[i] + dx;
      if (ys >= 0 && ys < H && xs >= 0 && xs < W) {
        const T* p = x + (((int64_t)rb[i] * H + ys) * W + xs) * Cin + c0;
        ra[i] = reinterpret_cast<const uint4*>(p)[chunk];
      } else {
        ra[i] = make_uint4(0, 0, 0, 0);
      }
    }
#pragma unroll
    for (int j = 0; j < WN; ++j) {
      const int n = n0 + rbase + 64 * j;
      if (n < Cout) rw[j] = reinterpret_cast<const uint4*>(w + (int64_t)n * K + t * Cin + c0)[chunk];
      else rw[j] = make_uint4(0, 0, 0, 0);
    }
  };

  f32x16_t acc[WM][WN];
#pragma unroll
  for (int i = 0; i < WM; ++i)
#pragma unroll
    for (int j = 0; j < WN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  unsigned char* As = lds;
  unsigned char* Bs = lds + BM * CV_ROWB;
  load(0);
  for (int s = 0; s < nslab; ++s) {
    __syncthreads();                                             // the previous slab's reads are done
#pragma unroll
    for (int i = 0; i < WM; ++i) *reinterpret_cast<uint4*>(As + (rbase + 64 * i) * CV_ROWB + 16 * chunk) = ra[i];
#pragma unroll
    for (int j = 0; j < WN; ++j) *reinterpret_cast<uint4*>(Bs + (rbase + 64 * j) * CV_ROWB + 16 * chunk) = rw[j];
    __syncthreads();
    if (s + 1 < nslab) load(s + 1);                              // in flight under this slab's MFMAs
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {                             // two 32-byte halves of the 64-byte slab
      uint4 fa[WM], fb[WN];
#pragma unroll
      for (int i = 0; i < WM; ++i)
        fa[i] = *reinterpret_cast<const uint4*>(As + (wm * WM * 32 + i * 32 + l31) * CV_ROWB + 32 * kk + 16 * half);
#pragma unroll
      for (int j = 0; j < WN; ++j)
        fb[j] = *reinterpret_cast<const uint4*>(Bs + (wn * WN * 32 + j * 32 + l31) * CV_ROWB + 32 * kk + 16 * half);
#pragma unroll
      for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j) acc[i][j] = cv_mfma<T>(fa[i], fb[j], acc[i][j]);
    }
  }

  // epilogue: acc[i][j][r] = D[(r & 3) + 8 (r >> 2) + 4 half][l31] of tile (i, j)
#pragma unroll
  for (int j = 0; j < WN; ++j) {
    const int n = n0 + wn * WN * 32 + j * 32 + l31;
    if (n >= Cout) continue;
    const float bn = bias[n];
#pragma unroll
    for (int i = 0; i < WM; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t m = m0 + wm * WM * 32 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (m >= M) continue;
        float v = acc[i][j][r] + bn;
        if (resid) v += ActIO<T>::ld(resid + m * Cout + n);
        if (relu) v = v < 0.f ? 0.f : v;
        ActIO<T>::st(y + m * Cout + n, v);
      }
    }
  }
}

// Stem conv1 (clip/model.py:101): 3x3, stride 2, pad 1, Cin 3, read from the fp32 NCHW image; w [Cout][3][3][3]
// (ky, kx, c) in the act dtype, staged in LDS as fp32.  One output pixel per thread, all Cout channels.
template <typename T>
__global__ __launch_bounds__(256) void stem_kernel(const float* __restrict__ img, const T* __restrict__ w,
                                                   const float* __restrict__ bias, T* y, int B, int H, int W, int Cout,
                                                   int relu) {
  __shared__ float ws[128 * 27];
  __shared__ float bs[128];
  for (int i = threadIdx.x; i < Cout * 27; i += blockDim.x) ws[i] = ActIO<T>::ld(w + i);
  for (int i = threadIdx.x; i < Cout; i += blockDim.x) bs[i] = bias[i];
  __syncthreads();
  const int Ho = H / 2, Wo = W / 2;
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (int64_t)B * Ho * Wo) return;
  const int b = (int)(p / ((int64_t)Ho * Wo));
  const int q = (int)(p - (int64_t)b * Ho * Wo), oy = q / Wo, ox = q - oy * Wo;
  float in[27];
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int iy = 2 * oy - 1 + ky, ix = 2 * ox - 1 + kx;
      const bool ok = iy >= 0 && iy < H && ix >= 0 && ix < W;
#pragma unroll
      for (int c = 0; c < 3; ++c)
        in[(ky * 3 + kx) * 3 + c] = ok ? img[(((int64_t)b * 3 + c) * H + iy) * W + ix] : 0.f;
    }
  T* out = y + p * Cout;
  for (int c0 = 0; c0 < Cout; c0 += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const float* wr = ws + (c0 + u) * 27;
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < 27; ++k) s = fmaf(in[k], wr[k], s);
      s += bs[c0 + u];
      v[u] = (relu && s < 0.f) ? 0.f : s;
    }
    Vec8<T>::st(out + c0, v);
  }
}

// AvgPool2d(k) on NHWC: one thread per (output pixel, 8 channels); sum over (dy, dx) in row order, divided by k*k.
template <typename T>
__global__ __launch_bounds__(256) void avgpool_kernel(const T* __restrict__ x, T* y, int B, int H, int W, int C, int k) {
  const int Ho = H / k, Wo = W / k, C8 = C / 8;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)B * Ho * Wo * C8) return;
  const int c = (int)(t % C8) * 8;
  const int64_t p = t / C8;
  const int b = (int)(p / ((int64_t)Ho * Wo));
  const int q = (int)(p - (int64_t)b * Ho * Wo), oy = q / Wo, ox = q - oy * Wo;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int dy = 0; dy < k; ++dy)
    for (int dx = 0; dx < k; ++dx) {
      float v[8];
      Vec8<T>::ld(x + (((int64_t)b * H + oy * k + dy) * W + ox * k + dx) * C + c, v);
#pragma unroll
      for (int u = 0; u < 8; ++u) s[u] += v[u];
    }
  const float inv = 1.0f / (float)(k * k);
#pragma unroll
  for (int u = 0; u < 8; ++u) s[u] = s[u] * inv;
  Vec8<T>::st(y + p * C + c, s);
}

// tokens[b][0] = mean_p x[b][p] + pos[0]; tokens[b][1 + p] = x[b][p] + pos[1 + p].  One thread per (image, 8 channels).
template <typename T>
__global__ __launch_bounds__(256) void tokens_kernel(const T* __restrict__ x, const float* __restrict__ pos, T* tok,
                                                     int B, int HW, int C) {
  const int C8 = C / 8;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= B * C8) return;
  const int b = t / C8, c = (t - b * C8) * 8;
  const T* xb = x + (int64_t)b * HW * C + c;
  T* tb = tok + (int64_t)b * (HW + 1) * C + c;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int p = 0; p < HW; ++p) {
    float v[8];
    Vec8<T>::ld(xb + (int64_t)p * C, v);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      s[u] += v[u];
      v[u] += pos[(int64_t)(1 + p) * C + c + u];
    }
    Vec8<T>::st(tb + (int64_t)(1 + p) * C, v);
  }
#pragma unroll
  for (int u = 0; u < 8; ++u) s[u] = s[u] / (float)HW + pos[c + u];
  Vec8<T>::st(tb, s);
}

// One wave per (head, image): scores of the scaled query against the T keys (lane j: key j, j + 64, ...), fp32 softmax,
// out[d = lane] = sum_j p_j v[j][d] / sum_j p_j in key order.  kv [B*T][2C] = (k | v) of every token, q [B][ldq] fp32.
template <typename T>
__global__ __launch_bounds__(64) void attnpool_kernel(const float* __restrict__ q, int64_t ldq, const T* __restrict__ kv,
                                                      T* out, int T_, int C, float scale) {
  __shared__ float qs[64];
  __shared__ float ps[CV_MAX_T];
  const int lane = threadIdx.x, h = blockIdx.x, b = blockIdx.y;
  qs[lane] = q[(int64_t)b * ldq + h * 64 + lane] * scale;
  __syncthreads();
  const T* kb = kv + (int64_t)b * T_ * 2 * C + h * 64;
  float mx = -INFINITY;
  for (int j = lane; j < T_; j += 64) {
    const T* kr = kb + (int64_t)j * 2 * C;
    float s = 0.f;
    for (int d = 0; d < 64; d += 8) {
      float v[8];
      Vec8<T>::ld(kr + d, v);
#pragma unroll
      for (int u = 0; u < 8; ++u) s = fmaf(qs[d + u], v[u], s);
    }
    ps[j] = s;
    mx = fmaxf(mx, s);
  }
  mx = wave_max(mx);
  float sum = 0.f;
  for (int j = lane; j < T_; j += 64) {
    const float e = __expf(ps[j] - mx);
    ps[j] = e;
    sum += e;
  }
  sum = wave_sum(sum);
  __syncthreads();
  float o = 0.f;
  const T* vb = kb + C;
  for (int j = 0; j < T_; ++j) o = fmaf(ps[j], ActIO<T>::ld(vb + (int64_t)j * 2 * C + lane), o);
  ActIO<T>::st(out + (int64_t)b * C + h * 64 + lane, o / sum);
}

template <int WM, int WN, typename T>
void launch_conv(const void* x, const void* w, const float* bias, const void* resid, void* y, int B, int H, int W,
                 int Cin, int Cout, int ks, int relu, hipStream_t s) {
  const int64_t M = (int64_t)B * H * W;
  const dim3 grid((unsigned)((M + 64 * WM - 1) / (64 * WM)), (unsigned)((Cout + 64 * WN - 1) / (64 * WN)));
  hipLaunchKernelGGL((conv_kernel<T, WM, WN>), grid, dim3(256), 0, s, static_cast<const T*>(x), static_cast<const T*>(w),
                     bias, static_cast<const T*>(resid), static_cast<T*>(y), B, H, W, Cin, Cout, ks, relu);
}

template <typename T>
void conv_dispatch(int cfg, const void* x, const void* w, const float* bias, const void* resid, void* y, int B, int H,
                   int W, int Cin, int Cout, int ks, int relu, hipStream_t s) {
  if (cfg == 2) launch_conv<2, 2, T>(x, w, bias, resid, y, B, H, W, Cin, Cout, ks, relu, s);
  else if (cfg == 3) launch_conv<2, 1, T>(x, w, bias, resid, y, B, H, W, Cin, Cout, ks, relu, s);
  else launch_conv<1, 1, T>(x, w, bias, resid, y, B, H, W, Cin, Cout, ks, relu, s);
}

bool dtype_ok(int dt) { return dt == RPO_F32 || dt == RPO_BF16 || dt == RPO_F16; }

}  // namespace

// 64 x 64 tiles for every shape.  Measured on the RN50 forward at batch 100, bf16 (profiles/rn_bench.json): every conv on
// 64 x 64 4.55 ms, on 128 x 64 4.70 ms, on 128 x 128 5.67 ms, and 5.24 ms for a rule that took the largest tile still
// giving two rounds of the CUs.  The larger tiles hold 2-4x the accumulators and leave 3-5 waves per SIMD instead of 8,
// too few to hide the gather loads of the single-buffered k loop.
extern "C" int rpo_conv2d_plan(int B, int H, int W, int Cout) {
  if (B <= 0 || H <= 0 || W <= 0 || Cout <= 0) return RPO_E_BADARG;
  return 1;
}

extern "C" int rpo_conv2d_nhwc(const void* x, const void* w, const float* bias, const void* resid, void* y, int dtype,
                               int B, int H, int W, int Cin, int Cout, int ksize, int relu, int tile_config,
                               void* stream) {
  if (!x || !w || !bias || !y || B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || !dtype_ok(dtype)) return RPO_E_BADARG;
  const int ck = dtype == RPO_F32 ? 16 : 32;
  if ((ksize != 1 && ksize != 3) || Cin % ck != 0 || Cout % 32 != 0) return RPO_E_SHAPE;
  if ((int64_t)B * H * W >= (int64_t)1 << 31 || (int64_t)ksize * ksize * Cin >= (int64_t)1 << 24) return RPO_E_SHAPE;
  if (tile_config < 0 || tile_config > 3) return RPO_E_BADARG;
  if (!aligned16(x) || !aligned16(w) || !aligned16(y) || (resid && !aligned16(resid))) return RPO_E_ALIGN;
  const int cfg = tile_config ? tile_config : rpo_conv2d_plan(B, H, W, Cout);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dtype == RPO_F32) conv_dispatch<float>(cfg, x, w, bias, resid, y, B, H, W, Cin, Cout, ksize, relu, s);
  else if (dtype == RPO_BF16) conv_dispatch<bf16_t>(cfg, x, w, bias, resid, y, B, H, W, Cin, Cout, ksize, relu, s);
  else conv_dispatch<f16_t>(cfg, x, w, bias, resid, y, B, H, W, Cin, Cout, ksize, relu, s);
  return rpo_launch_status();
}

extern "C" int rpo_conv_stem(const float* image, const void* w, const float* bias, void* y, int dtype, int B, int H,
                             int W, int Cout, int relu, void* stream) {
  if (!image || !w || !bias || !y || B <= 0 || H <= 0 || W <= 0 || Cout <= 0 || !dtype_ok(dtype)) return RPO_E_BADARG;
  if (H % 2 || W % 2 || Cout % 8 || Cout > 128 || (int64_t)B * H * W >= (int64_t)1 << 31) return RPO_E_SHAPE;
  if (!aligned16(y)) return RPO_E_ALIGN;
  const int64_t P = (int64_t)B * (H / 2) * (W / 2);
  const dim3 grid((unsigned)((P + 255) / 256));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dtype == RPO_F32)
    hipLaunchKernelGGL(stem_kernel<float>, grid, dim3(256), 0, s, image, static_cast<const float*>(w), bias,
                       static_cast<float*>(y), B, H, W, Cout, relu);
  else if (dtype == RPO_BF16)
    hipLaunchKernelGGL(stem_kernel<bf16_t>, grid, dim3(256), 0, s, image, static_cast<const bf16_t*>(w), bias,
                       static_cast<bf16_t*>(y), B, H, W, Cout, relu);
  else
    hipLaunchKernelGGL(stem_kernel<f16_t>, grid, dim3(256), 0, s, image, static_cast<const f16_t*>(w), bias,
                       static_cast<f16_t*>(y), B, H, W, Cout, relu);
  return rpo_launch_status();
}

extern "C" int rpo_avgpool_nhwc(const void* x, void* y, int dtype, int B, int H, int W, int C, int k, void* stream) {
  if (!x || !y || B <= 0 || H <= 0 || W <= 0 || C <= 0 || k <= 0 || !dtype_ok(dtype)) return RPO_E_BADARG;
  if (H % k || W % k || C % 8 || (int64_t)B * H * W * C >= (int64_t)1 << 40) return RPO_E_SHAPE;
  if (!aligned16(x) || !aligned16(y)) return RPO_E_ALIGN;
  const int64_t n = (int64_t)B * (H / k) * (W / k) * (C / 8);
  const dim3 grid((unsigned)((n + 255) / 256));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dtype == RPO_F32)
    hipLaunchKernelGGL(avgpool_kernel<float>, grid, dim3(256), 0, s, static_cast<const float*>(x), static_cast<float*>(y),
                       B, H, W, C, k);
  else if (dtype == RPO_BF16)
    hipLaunchKernelGGL(avgpool_kernel<bf16_t>, grid, dim3(256), 0, s, static_cast<const bf16_t*>(x),
                       static_cast<bf16_t*>(y), B, H, W, C, k);
  else
    hipLaunchKernelGGL(avgpool_kernel<f16_t>, grid, dim3(256), 0, s, static_cast<const f16_t*>(x),
                       static_cast<f16_t*>(y), B, H, W, C, k);
  return rpo_launch_status();
}

extern "C" int rpo_attnpool_tokens(const void* x, const float* pos, void* tokens, int dtype, int B, int HW, int C,
                                   void* stream) {
  if (!x || !pos || !tokens || B <= 0 || HW <= 0 || C <= 0 || !dtype_ok(dtype)) return RPO_E_BADARG;
  if (C % 8 || HW + 1 > CV_MAX_T || (int64_t)B * C >= (int64_t)1 << 30) return RPO_E_SHAPE;
  if (!aligned16(x) || !aligned16(tokens)) return RPO_E_ALIGN;
  const int n = B * (C / 8);
  const dim3 grid((unsigned)((n + 255) / 256));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dtype == RPO_F32)
    hipLaunchKernelGGL(tokens_kernel<float>, grid, dim3(256), 0, s, static_cast<const float*>(x), pos,
                       static_cast<float*>(tokens), B, HW, C);
  else if (dtype == RPO_BF16)
    hipLaunchKernelGGL(tokens_kernel<bf16_t>, grid, dim3(256), 0, s, static_cast<const bf16_t*>(x), pos,
                       static_cast<bf16_t*>(tokens), B, HW, C);
  else
    hipLaunchKernelGGL(tokens_kernel<f16_t>, grid, dim3(256), 0, s, static_cast<const f16_t*>(x), pos,
                       static_cast<f16_t*>(tokens), B, HW, C);
  return rpo_launch_status();
}

extern "C" int rpo_attnpool_attn(const float* q, int64_t ldq, const void* kv, void* out, int dtype, int B, int T, int C,
                                 int heads, float scale, void* stream) {
  if (!q || !kv || !out || B <= 0 || T <= 0 || C <= 0 || heads <= 0 || ldq < C || !dtype_ok(dtype)) return RPO_E_BADARG;
  if (C != 64 * heads || T > CV_MAX_T || B > 65535) return RPO_E_SHAPE;
  if (!aligned16(kv)) return RPO_E_ALIGN;
  const dim3 grid(heads, B);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dtype == RPO_F32)
    hipLaunchKernelGGL(attnpool_kernel<float>, grid, dim3(64), 0, s, q, ldq, static_cast<const float*>(kv),
                       static_cast<float*>(out), T, C, scale);
  else if (dtype == RPO_BF16)
    hipLaunchKernelGGL(attnpool_kernel<bf16_t>, grid, dim3(64), 0, s, q, ldq, static_cast<const bf16_t*>(kv),
                       static_cast<bf16_t*>(out), T, C, scale);
  else
    hipLaunchKernelGGL(attnpool_kernel<f16_t>, grid, dim3(64), 0, s, q, ldq, static_cast<const f16_t*>(kv),
                       static_cast<f16_t*>(out), T, C, scale);
  return rpo_launch_status();
}
