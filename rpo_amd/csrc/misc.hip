// Small HBM-bound kernels around the towers: patch im2col, token-matrix assembly, prompt
// broadcast / gradient reduction, cosine-logit head + cross-entropy (fwd and bwd), SGD,
// dtype conversion, and the MFMA layout probe used by the test-suite.
#include "common.h"

namespace {

// ---- im2col for non-overlapping patches (trainers/rpo.py:198-200) -------------------------
// one thread per 2 consecutive pixels of an image row (8-B fp32 load, packed store); threads of a
// wave cover consecutive pixels of the image row, so loads coalesce.  Requires patch % 2 == 0.
template <typename TO>
__global__ void im2col_kernel(const float* __restrict__ img, TO* out, int64_t ldo, int B, int H, int W,
                              int p, int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // ((b*3 + c)*H + y) * (W/2) + x2
  if (idx >= total) return;
  const int w2 = W >> 1;
  const int x = (int)(idx % w2) * 2;
  const int64_t row = idx / w2;
  const int y = (int)(row % H);
  const int c = (int)((row / H) % 3);
  const int b = (int)(row / (3 * (int64_t)H));
  const float2 v = *reinterpret_cast<const float2*>(img + row * W + x);
  const int g = W / p;
  const int py = y / p, ky = y - py * p, px = x / p, kx = x - px * p;
  const int64_t m = ((int64_t)b * (H / p) + py) * g + px;
  TO* dst = out + m * ldo + (c * p + ky) * p + kx;
  ActIO<TO>::st(dst, v.x);
  ActIO<TO>::st(dst + 1, v.y);
  if (c == 2 && ky == p - 1 && kx + 2 >= p)       // last pixels of the patch: zero the K padding
    for (int k = 3 * p * p; k < ldo; ++k) ActIO<TO>::st(out + m * ldo + k, 0.f);
}

// patch % 8 == 0 (ViT-B/16, /32): one thread per 8 consecutive pixels -- two 16-B loads, one 16-B store in the 16-bit
// modes (the 2-pixel version above issues 4-B stores: 15 us for the 19 MB image batch at B = 32, this one 3x fewer
// instructions per byte).  Same values, same layout.
template <typename TO>
__global__ void im2col8_kernel(const float* __restrict__ img, TO* out, int64_t ldo, int B, int H, int W,
                               int p, int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // ((b*3 + c)*H + y) * (W/8) + x8
  if (idx >= total) return;
  const int w8 = W >> 3;
  const int x = (int)(idx % w8) * 8;
  const int64_t row = idx / w8;
  const int y = (int)(row % H);
  const int c = (int)((row / H) % 3);
  const int b = (int)(row / (3 * (int64_t)H));
  const float4 v0 = *reinterpret_cast<const float4*>(img + row * W + x);
  const float4 v1 = *reinterpret_cast<const float4*>(img + row * W + x + 4);
  const int g = W / p;
  const int py = y / p, ky = y - py * p, px = x / p, kx = x - px * p;
  const int64_t m = ((int64_t)b * (H / p) + py) * g + px;
  TO* dst = out + m * ldo + (c * p + ky) * p + kx;
  if constexpr (sizeof(TO) == 2) {
    uint4 o;
    o.x = pack2<TO>(v0.x, v0.y); o.y = pack2<TO>(v0.z, v0.w);
    o.z = pack2<TO>(v1.x, v1.y); o.w = pack2<TO>(v1.z, v1.w);
    *reinterpret_cast<uint4*>(dst) = o;
  } else {
    *reinterpret_cast<float4*>(dst) = v0;
    *reinterpret_cast<float4*>(dst + 4) = v1;
  }
  if (c == 2 && ky == p - 1 && kx + 8 >= p)       // last pixels of the patch: zero the K padding
    for (int k = 3 * p * p; k < ldo; ++k) ActIO<TO>::st(out + m * ldo + k, 0.f);
}

__global__ void assemble_kernel(float* x, int64_t ldx, const float* __restrict__ cls,
                                const float* __restrict__ pos0, const float* __restrict__ prompt, int B, int N,
                                int Kp, int d) {
  const int r = blockIdx.x;                 // 0..B-1: CLS rows; B.. : prompt rows
  float* dst;
  if (r < B) {
    dst = x + (int64_t)r * N * ldx;
    for (int i = threadIdx.x; i < d; i += blockDim.x) dst[i] = cls[i] + pos0[i];
  } else {
    const int pr = r - B;                   // b*Kp + i
    dst = x + ((int64_t)B * N + pr) * ldx;
    const float* src = prompt + (int64_t)(pr % Kp) * d;
    for (int i = threadIdx.x; i < d; i += blockDim.x) dst[i] = src[i];
  }
}

__global__ void broadcast_rows_kernel(const float* __restrict__ src, float* dst, int64_t ld, int rows, int d,
                                      int set_rows, int64_t src_stride) {
  const int r = blockIdx.x;                 // (s*groups + g)*rows + i; set_rows = groups * rows (one set: s = 0)
  const float* s = src + (int64_t)(r / set_rows) * src_stride + (int64_t)(r % rows) * d;
  float* o = dst + (int64_t)r * ld;
  for (int i = threadIdx.x; i < d; i += blockDim.x) o[i] = s[i];
}

// Token embedding + positional embedding of a text pass's input rows (make_prompts, trainers/rpo.py:135-136; CoOp's
// context slots, trainers/coop.py:136-183), gathered on the device: pure byte work, 2 reads + 1 write of rows * d floats.
// One workgroup per row under a grid-stride loop: the row's id is one load at a workgroup-uniform address, every lane
// moves 16 bytes per access, no LDS.  An id is clamped into its table, so no id reads outside the arguments.
__global__ __launch_bounds__(128) void text_embed_kernel(const int32_t* __restrict__ ids, int64_t ld_ids,
                                                         const float4* __restrict__ table, int vocab,
                                                         const float4* __restrict__ pos, const float4* __restrict__ ctx,
                                                         int n_ctx, float4* __restrict__ out, int64_t rows, int L, int d4) {
  for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
    const int64_t c = r / L;
    const int p = (int)(r - c * L);
    const int id = ids[c * ld_ids + p];
    const float4* src;
    if (id < 0 && n_ctx > 0) src = ctx + (int64_t)min(-1 - id, n_ctx - 1) * d4;
    else src = table + (int64_t)min(max(id, 0), vocab - 1) * d4;
    const float4* pe = pos + (int64_t)p * d4;
    float4* o = out + r * d4;
    for (int i = threadIdx.x; i < d4; i += 128) {
      const float4 a = src[i], b = pe[i];
      o[i] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
    }
  }
}

__global__ void reduce_groups_kernel(const float* __restrict__ src, int64_t ld, float* out, int groups, int rows,
                                     int d, int64_t out_stride) {
  src += (int64_t)blockIdx.y * groups * rows * ld;                  // blockIdx.y: the set (rpo_reduce_groups_sets)
  out += (int64_t)blockIdx.y * out_stride;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= rows * d) return;
  const int i = idx / d, c = idx % d;
  float s = 0.f;
  for (int g = 0; g < groups; ++g) s += src[((int64_t)g * rows + i) * ld + c];
  out[idx] = s;
}

// Many groups (the text tower's prompt gradient summed over hundreds of classes: 1000 x [24, 512] at ImageNet): the kernel
// above is rows * d threads each walking `groups` strided loads one after the other (460 us at 1000 groups).  Here a
// block of 256 threads owns 32 consecutive columns of one row and splits the GROUPS over its 8 thread rows (thread row j
// sums groups j, j + 8, ... in ascending order), then adds the 8 partial sums in thread-row order through LDS: a fixed
// summation order (deterministic), 8 x the loads in flight and 8 x the workgroups.
__global__ __launch_bounds__(256) void reduce_groups_wide_kernel(const float* __restrict__ src, int64_t ld, float* out,
                                                                 int groups, int rows, int d, int64_t out_stride) {
  __shared__ float part[8][32];
  src += (int64_t)blockIdx.y * groups * rows * ld;                  // blockIdx.y: the set (rpo_reduce_groups_sets)
  out += (int64_t)blockIdx.y * out_stride;
  const int cols = (d + 31) / 32;
  const int i = blockIdx.x / cols, c = (blockIdx.x % cols) * 32 + (threadIdx.x & 31), j = threadIdx.x >> 5;
  float s = 0.f;
  if (c < d)
    for (int g = j; g < groups; g += 8) s += src[((int64_t)g * rows + i) * ld + c];
  part[j][threadIdx.x & 31] = s;
  __syncthreads();
  if (j == 0 && c < d) {
    float t = part[0][threadIdx.x];
#pragma unroll
    for (int k = 1; k < 8; ++k) t += part[k][threadIdx.x];
    out[(int64_t)i * d + c] = t;
  }
}

__global__ void sgd_kernel(float* p, const float* __restrict__ g, float* buf, int64_t n, float lr, float mom,
                           float wd, float gs, int first) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float pi = p[i];
  const float gi = gs * g[i] + wd * pi;
  const float bi = first ? gi : mom * buf[i] + gi;
  buf[i] = bi;
  p[i] = pi - lr * bi;
}

// The same step as GradScaler.step would take it (trainers/rpo.py:298-304, PREC amp): skipped as a whole when any gradient
// is Inf / NaN.  One workgroup: the scan has to finish before the first update, and the trainable state is 30 720 floats.
// found[0] = this step's flag, found[1] += 1 per skipped step.  The momentum buffer must start at zero: a skipped first
// step then leaves the next one in the state torch's first step starts from.
__global__ __launch_bounds__(1024) void sgd_guarded_kernel(float* p, const float* __restrict__ g, float* buf, int64_t n,
                                                           float lr, float mom, float wd, float gs, int first,
                                                           int32_t* found) {
  __shared__ int bad;
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  int mine = 0;
  for (int64_t i = threadIdx.x; i < n; i += 1024) {
    const float gi = g[i];
    mine |= !(fabsf(gi) <= 3.402823466e38f);                        // Inf or NaN
  }
  if (mine) bad = 1;
  __syncthreads();
  const int skip = bad;
  if (threadIdx.x == 0) { found[0] = skip; found[1] += skip; }
  if (skip) return;
  for (int64_t i = threadIdx.x; i < n; i += 1024) {
    const float pi = p[i];
    const float gi = gs * g[i] + wd * pi;
    const float bi = first ? gi : mom * buf[i] + gi;
    buf[i] = bi;
    p[i] = pi - lr * bi;
  }
}

// rpo_sgd_step_sets: the two kernels above with the set (blockIdx.y / blockIdx.x) as the outer index, the four scalars
// read from the set's row of `hyper` (lr, momentum, weight decay, grad_scale) and the element range cut to the leading
// used[set] = (u0, u1) floats of the segments [0, seg0) and [seg0, seg0 + seg1) of the set's row.  The update is written as
// in sgd_kernel, so that it contracts to the same instructions: per element the bits of rpo_sgd_step[_guarded].
__device__ __forceinline__ bool sgd_set_uses(int64_t i, int64_t seg0, int64_t u0, int64_t u1) {
  return i < seg0 ? i < u0 : i - seg0 < u1;
}
__device__ __forceinline__ void sgd_set_ranges(const int32_t* used, int set, int64_t seg0, int64_t seg1, int64_t& u0,
                                               int64_t& u1) {
  u0 = seg0; u1 = seg1;
  if (used != nullptr) {
    u0 = min(max((int64_t)used[2 * set], (int64_t)0), seg0);
    u1 = min(max((int64_t)used[2 * set + 1], (int64_t)0), seg1);
  }
}

__global__ void sgd_sets_kernel(float* p, const float* __restrict__ g, float* buf, int64_t set_stride,
                                const float* __restrict__ hyper, const int32_t* __restrict__ used, int64_t seg0,
                                int64_t seg1, int first) {
  const int set = blockIdx.y;
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= seg0 + seg1) return;
  int64_t u0, u1;
  sgd_set_ranges(used, set, seg0, seg1, u0, u1);
  if (!sgd_set_uses(j, seg0, u0, u1)) return;
  const float lr = hyper[4 * set], mom = hyper[4 * set + 1], wd = hyper[4 * set + 2], gs = hyper[4 * set + 3];
  const int64_t i = (int64_t)set * set_stride + j;
  const float pi = p[i];
  const float gi = gs * g[i] + wd * pi;
  const float bi = first ? gi : mom * buf[i] + gi;
  buf[i] = bi;
  p[i] = pi - lr * bi;
}

__global__ __launch_bounds__(1024) void sgd_sets_guarded_kernel(float* p, const float* __restrict__ g, float* buf,
                                                                int64_t set_stride, const float* __restrict__ hyper,
                                                                const int32_t* __restrict__ used, int64_t seg0,
                                                                int64_t seg1, int first, int32_t* found) {
  __shared__ int bad;
  const int set = blockIdx.x;
  p += (int64_t)set * set_stride; g += (int64_t)set * set_stride; buf += (int64_t)set * set_stride; found += 2 * set;
  int64_t u0, u1;
  sgd_set_ranges(used, set, seg0, seg1, u0, u1);
  const int64_t n = seg0 + seg1;
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  int mine = 0;
  for (int64_t i = threadIdx.x; i < n; i += 1024) {
    if (!sgd_set_uses(i, seg0, u0, u1)) continue;
    const float gi = g[i];
    mine |= !(fabsf(gi) <= 3.402823466e38f);                        // Inf or NaN
  }
  if (mine) bad = 1;
  __syncthreads();
  const int skip = bad;
  if (threadIdx.x == 0) { found[0] = skip; found[1] += skip; }
  if (skip) return;
  const float lr = hyper[4 * set], mom = hyper[4 * set + 1], wd = hyper[4 * set + 2], gs = hyper[4 * set + 3];
  for (int64_t i = threadIdx.x; i < n; i += 1024) {
    if (!sgd_set_uses(i, seg0, u0, u1)) continue;
    const float pi = p[i];
    const float gi = gs * g[i] + wd * pi;
    const float bi = first ? gi : mom * buf[i] + gi;
    buf[i] = bi;
    p[i] = pi - lr * bi;
  }
}

template <typename TO>
__global__ void convert_kernel(const float* __restrict__ src, int64_t lds, TO* dst, int64_t ldd, int rows,
                               int cols) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)rows * cols) return;
  const int64_t r = idx / cols, c = idx % cols;
  ActIO<TO>::st(dst + r * ldd + c, src[r * lds + c]);
}

// ---- head ---------------------------------------------------------------------------------
__device__ __forceinline__ float block_sum(float v, float* red) {  // 256 threads
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// logits[b,c] = (scale/K) * sum_i <x_i, t_i> / (|x_i| |t_i|)   (trainers/rpo.py:215-227), x_i = img_f[b,i], t_i = text_f[c,i].
// One block per (class, image): B * C independent blocks (608 for the Oxford-Pets base split at B = 32), wave w takes the
// pairs i = w, w+4, ...; a pair is one pass over both raw rows accumulating <x,t>, |x|^2 and |t|^2 -- no separate
// normalisation launch, no unit-vector copies.  The inverse norms the backward needs are left in ni / nt by the blocks of
// class 0 / image 0.  (A version with one block per image that looped over all C * K text rows took 150 us: 120 dependent
// load -> reduce rounds per wave on 32 CUs.)
// Several independent heads in one launch (rpo_head_fwd_bwd_grouped): group s pairs images [s B, (s + 1) B) with text
// features [s C, (s + 1) C) only.  Every kernel below takes the group from a grid dimension and moves its pointers by the
// group's strides (elements) before doing exactly what it does for a single head; a single head is group 0 of 1.
struct HeadGroups {
  int64_t img;      // B * K * e   (img_f, d_img_f, their act copies)
  int64_t txt;      // C * K * e   (text_f, d_text_f, their act copies)
  int64_t bc;       // B * C       (logits)
  int64_t lab;      // B           (label)
  int64_t ws;       // workspace floats per group (rpo_head_workspace_floats)
  const int32_t* k; // rpo_head_fwd_bwd_grouped_k: pairs in use per group (device, [S]); NULL: all K in every group
  float scale_exp;  // (read only with k: the group's own scale_exp / k and scale_exp / (k B))
};
template <typename T> __device__ __forceinline__ T* head_shift(T* p, int64_t off) { return p == nullptr ? p : p + off; }
__device__ __forceinline__ void* head_shift16(void* p, int64_t off) {            // act copies: 2-byte elements
  return p == nullptr ? p : static_cast<void*>(static_cast<uint16_t*>(p) + off);
}
// Per-group K (rpo_head_fwd_bwd_grouped_k): group s pairs only its first k = hg.k[s] of the K rows per image / class.  Every
// kernel below bounds its pair index by head_k instead of K and takes the two factors that hold K from head_mul / head_gmul;
// the strides stay those of K rows.  Rows i >= k are never read; their gradient rows are written as zeros (head_fill).  A k
// outside [1, K] counts as 0 pairs with NaN factors: that group's logits, loss and gradients are NaN, nothing is read.
// PK: the kernel instance of rpo_head_fwd_bwd_grouped_k.  The existing entry points launch the <.., false> instances, in which
// all of this folds away: their code is what it was.
template <bool PK> __device__ __forceinline__ int head_k(const HeadGroups& hg, int64_t s, int K) {
  if constexpr (!PK) return K;
  const int k = hg.k[s];
  return k >= 1 && k <= K ? k : 0;
}
template <bool PK> __device__ __forceinline__ float head_mul(const HeadGroups& hg, int k, float mul) {     // scale_exp / k
  if constexpr (!PK) return mul;
  return k > 0 ? hg.scale_exp / (float)k : __builtin_nanf("");
}
template <bool PK> __device__ __forceinline__ float head_gmul(const HeadGroups& hg, int k, float gmul) {   // scale_exp / (k B)
  if constexpr (!PK) return gmul;
  return k > 0 ? hg.scale_exp / ((float)k * (float)hg.lab) : __builtin_nanf("");
}
__device__ __forceinline__ float head_fill(int k) { return k > 0 ? 0.0f : __builtin_nanf(""); }

__device__ __forceinline__ void head_store(float* df, void* da, int act_dtype, int64_t off, float g) {
  df[off] = g;
  if (da != nullptr) {                       // the act-dtype copy the dX GEMM of the projection reads (RNE, as rpo_convert)
    if (act_dtype == RPO_BF16) reinterpret_cast<uint16_t*>(da)[off] = (uint16_t)(pack2<bf16_t>(g, 0.f) & 0xffffu);
    else reinterpret_cast<uint16_t*>(da)[off] = (uint16_t)(pack2<f16_t>(g, 0.f) & 0xffffu);
  }
}

template <bool VEC, bool PK>
__global__ __launch_bounds__(256) void head_logits_kernel(const float* __restrict__ f_img, const float* __restrict__ f_txt,
                                                          float* ni, float* nt, float* logits, int C, int K, int e,
                                                          float mul, HeadGroups hg) {
  __shared__ float red[4];
  {
    const int64_t s = blockIdx.z;
    f_img += s * hg.img; f_txt += s * hg.txt; ni += s * hg.ws; nt += s * hg.ws; logits += s * hg.bc;
  }
  const int c = blockIdx.x, b = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ku = head_k<PK>(hg, blockIdx.z, K);
  mul = head_mul<PK>(hg, ku, mul);
  float acc = 0.f;
#pragma unroll 2
  for (int i = wave; i < ku; i += 4) {
    const float* x = f_img + ((int64_t)b * K + i) * e;
    const float* t = f_txt + ((int64_t)c * K + i) * e;
    float dot = 0.f, sx = 0.f, st = 0.f;
    if constexpr (VEC) {                                           // e % 256 == 0, e <= 1024: all loads in flight at once
      float4 xv[4], tv[4];
      const int nv = e >> 8;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < nv) {
          xv[j] = *reinterpret_cast<const float4*>(x + j * 256 + lane * 4);
          tv[j] = *reinterpret_cast<const float4*>(t + j * 256 + lane * 4);
        }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < nv) {
          dot += xv[j].x * tv[j].x + xv[j].y * tv[j].y + xv[j].z * tv[j].z + xv[j].w * tv[j].w;
          sx += xv[j].x * xv[j].x + xv[j].y * xv[j].y + xv[j].z * xv[j].z + xv[j].w * xv[j].w;
          st += tv[j].x * tv[j].x + tv[j].y * tv[j].y + tv[j].z * tv[j].z + tv[j].w * tv[j].w;
        }
    } else {
      for (int idx = lane; idx < e; idx += 64) {
        const float xv = x[idx], tv = t[idx];
        dot = fmaf(xv, tv, dot); sx = fmaf(xv, xv, sx); st = fmaf(tv, tv, st);
      }
    }
    dot = wave_sum(dot); sx = wave_sum(sx); st = wave_sum(st);
    const float ix = 1.0f / sqrtf(sx), it = 1.0f / sqrtf(st);
    acc += dot * ix * it;
    if (lane == 0) {
      if (c == 0) ni[(int64_t)b * K + i] = ix;
      if (b == 0) nt[(int64_t)c * K + i] = it;
    }
  }
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) logits[(int64_t)b * C + c] = ((red[0] + red[1]) + (red[2] + red[3])) * mul;
}

// per image: loss_b = logsumexp - logit[label]; dl[b,c] = (softmax - onehot) * gmul
template <bool PK>
__global__ __launch_bounds__(256) void head_ce_kernel(const float* __restrict__ logits,
                                                      const int64_t* __restrict__ label, float* dl,
                                                      float* loss_b, int C, float gmul, float* dlT, int B,
                                                      HeadGroups hg) {
  __shared__ float red[4];
  {
    const int64_t s = blockIdx.y;
    logits += s * hg.bc; label += s * hg.lab; dl += s * hg.ws; loss_b += s * hg.ws; dlT = head_shift(dlT, s * hg.ws);
    gmul = head_gmul<PK>(hg, head_k<PK>(hg, s, 1 << 30), gmul);
  }
  const int b = blockIdx.x;
  const float* z = logits + (int64_t)b * C;
  float m = -INFINITY;
  for (int c = threadIdx.x; c < C; c += 256) m = fmaxf(m, z[c]);
  m = block_max(m, red);
  float s = 0.f;
  for (int c = threadIdx.x; c < C; c += 256) s += expf(z[c] - m);
  s = block_sum(s, red);
  // F.cross_entropy (trainers/rpo.py:230) raises on an out-of-range target; a kernel cannot, so it neither reads
  // out of bounds nor returns a plausible number: the loss becomes NaN (hosts validate labels they can see)
  const int64_t lb64 = label[b];
  const bool lb_ok = lb64 >= 0 && lb64 < C;
  const int lb = lb_ok ? (int)lb64 : -1;
  const float inv = 1.0f / s;
  // ... and so do this image's dl weights, hence both prompt gradients: rpo_sgd_step_guarded / check_finite then see the
  // bad label instead of applying a finite-looking (softmax without its one-hot term) update
  const float poison = lb_ok ? 0.0f : __builtin_nanf("");
  for (int c = threadIdx.x; c < C; c += 256) {
    const float w = (expf(z[c] - m) * inv - (c == lb ? 1.0f : 0.0f)) * gmul + poison;
    dl[(int64_t)b * C + c] = w;
    if (dlT != nullptr) dlT[(int64_t)c * B + b] = w;               // (the MFMA backward of the image side reads it by class)
  }
  if (threadIdx.x == 0) loss_b[b] = lb_ok ? (m + logf(s)) - z[lb] : __builtin_nanf("");
}

// one block per feature row (g, i) of the "self" side; other side has `n_other` groups.
//   h = f / |f|;  dh[e] = sum_o dl(g,o) * other[o,i,e] / |other[o,i]|;  df = (dh - h * <h,dh>) / |f|
// Blocks [0, B*K) are the image rows (dl[g*C + o], o = class), blocks [B*K, B*K + C*K) the class rows
// (dl[o*C + g], o = image): both sides in ONE launch, from the raw features and the inverse norms of head_logits_kernel.
// FUSED_CE (class sets up to 128): there is no cross-entropy launch and no dl array -- every block recomputes the
// softmax statistics (max, 1 / sum) it needs from the logits (its own image's row, or all B rows for a class-row block:
// B * C <= a few thousand exps) and forms its dl weights in LDS; block 0 also writes the mean loss.  Fixed summation
// orders throughout.  F.cross_entropy (trainers/rpo.py:230) raises on an out-of-range target; a kernel cannot, so it
// neither reads out of bounds nor returns a plausible number: the loss becomes NaN (hosts validate labels they can see).
template <bool FUSED_CE, bool PK>
__global__ __launch_bounds__(256) void head_bwd_kernel(const float* __restrict__ dl, const float* __restrict__ f_img,
                                                       const float* __restrict__ ni, const float* __restrict__ f_txt,
                                                       const float* __restrict__ nt, float* d_img_f, float* d_text_f,
                                                       int B, int C, int K, int e, const float* loss_b, float* loss,
                                                       const float* __restrict__ logits,
                                                       const int64_t* __restrict__ label, float gmul,
                                                       void* d_img_a, void* d_text_a, int act_dtype, HeadGroups hg) {
  extern __shared__ __attribute__((aligned(16))) char head_smem[];
  __shared__ float red[4];
  {
    const int64_t s = blockIdx.y;
    dl += s * hg.ws; ni += s * hg.ws; nt += s * hg.ws; loss_b += s * hg.ws;
    f_img += s * hg.img; f_txt += s * hg.txt; d_img_f += s * hg.img; d_text_f += s * hg.txt;
    d_img_a = head_shift16(d_img_a, s * hg.img); d_text_a = head_shift16(d_text_a, s * hg.txt);
    logits += s * hg.bc; label = head_shift(label, s * hg.lab); loss = head_shift(loss, s);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool img = (int)blockIdx.x < B * K;
  const int row = img ? blockIdx.x : blockIdx.x - B * K;            // g*K + i
  const int g = row / K, i = row % K;
  const int ku = head_k<PK>(hg, blockIdx.y, K);
  if (PK && i >= ku) {                                              // a pair this group does not use: zeros, nothing read
    if (loss != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *loss = __builtin_nanf("");     // (i = 0: k out of range)
    void* da = img ? d_img_a : d_text_a;
    for (int idx = threadIdx.x; idx < e; idx += 256)
      head_store(img ? d_img_f : d_text_f, da, act_dtype, (int64_t)row * e + idx, head_fill(ku));
    return;
  }
  gmul = head_gmul<PK>(hg, ku, gmul);
  const float* self_raw = img ? f_img : f_txt;
  const float* self_inv = img ? ni : nt;
  const float* other_raw = img ? f_txt : f_img;
  const float* other_inv = img ? nt : ni;
  float* df = img ? d_img_f : d_text_f;
  const int n_other = img ? C : B;
  float* wts = reinterpret_cast<float*>(head_smem);               // [max(B, C)]  dl(g, o) / |other[o, i]|
  if constexpr (FUSED_CE) {
    float* smax = wts + max(B, C);                                  // [B]
    float* sinv = smax + B;                                         // [B]
    float* lrow = sinv + B;                                         // [B] per-image loss (block 0)
    const bool all = !img || blockIdx.x == 0;                       // statistics of every image, or of image g only
    for (int b = all ? wave : g + wave; b < (all ? B : g + 1); b += 4) {
      const float z0 = lane < C ? logits[(int64_t)b * C + lane] : -INFINITY;
      const float z1 = lane + 64 < C ? logits[(int64_t)b * C + lane + 64] : -INFINITY;
      const float m = wave_max(fmaxf(z0, z1));
      const float ssum = wave_sum((lane < C ? expf(z0 - m) : 0.f) + (lane + 64 < C ? expf(z1 - m) : 0.f));
      if (lane == 0) {
        smax[b] = m; sinv[b] = 1.0f / ssum;
        if (blockIdx.x == 0) {
          const int64_t lb = label[b];
          lrow[b] = lb >= 0 && lb < C ? (m + logf(ssum)) - logits[(int64_t)b * C + lb] : __builtin_nanf("");
        }
      }
    }
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x == 0) {                      // mean CE over the batch
      float s = 0.f;
      for (int b = 0; b < B; ++b) s += lrow[b];
      *loss = s / (float)B;
    }
    for (int o = threadIdx.x; o < n_other; o += 256) {
      const int b = img ? g : o, c = img ? o : g;
      const float p = expf(logits[(int64_t)b * C + c] - smax[b]) * sinv[b];
      const int64_t lb = label[b];
      // an out-of-range label poisons the weights (hence both prompt gradients), not only the loss: the guarded
      // optimiser step / check_finite must not apply a finite-looking update computed without the one-hot term
      const float poison = lb >= 0 && lb < C ? 0.0f : __builtin_nanf("");
      wts[o] = (p - (lb == (int64_t)c ? 1.0f : 0.0f)) * gmul * other_inv[(int64_t)o * K + i] + poison;
    }
  } else {
    if (loss != nullptr && blockIdx.x == 0 && threadIdx.x == 0) {  // mean CE over the batch, fixed summation order
      float s = 0.f;
      for (int b = 0; b < B; ++b) s += loss_b[b];
      *loss = s / (float)B;
    }
    const int64_t sg = img ? C : 1, so = img ? 1 : C;
    for (int o = threadIdx.x; o < n_other; o += 256) wts[o] = dl[g * sg + o * so] * other_inv[(int64_t)o * K + i];
  }
  __syncthreads();
  const float inv = self_inv[row];
  float h[4], dh[4] = {0.f, 0.f, 0.f, 0.f};                         // e <= 4 * 256 handled in registers
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int idx = threadIdx.x + 256 * v;
    h[v] = idx < e ? self_raw[(int64_t)row * e + idx] * inv : 0.f;
  }
#pragma unroll 4
  for (int o = 0; o < n_other; ++o) {
    const float w = wts[o];
    const float* y = other_raw + ((int64_t)o * K + i) * e;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int idx = threadIdx.x + 256 * v;
      if (idx < e) dh[v] = fmaf(w, y[idx], dh[v]);
    }
  }
  float dot = 0.f;
#pragma unroll
  for (int v = 0; v < 4; ++v) dot = fmaf(h[v], dh[v], dot);
  dot = block_sum(dot, red);
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int idx = threadIdx.x + 256 * v;
    if (idx < e) {
      const float g = (dh[v] - h[v] * dot) * inv;
      df[(int64_t)row * e + idx] = g;
      // the act-dtype copy the dX GEMM of the projection reads (RNE, as rpo_convert would make it)
      void* da = img ? d_img_a : d_text_a;
      if (da != nullptr) {
        if (act_dtype == RPO_BF16) reinterpret_cast<uint16_t*>(da)[(int64_t)row * e + idx] = (uint16_t)(pack2<bf16_t>(g, 0.f) & 0xffffu);
        else reinterpret_cast<uint16_t*>(da)[(int64_t)row * e + idx] = (uint16_t)(pack2<f16_t>(g, 0.f) & 0xffffu);
      }
    }
  }
}

// ---- head at large class counts (C > 128: SUN397, ImageNet's 1000) -------------------------------------------------------
// The kernels above give every (class, image) pair / every feature row its own block, each re-reading the rows of the other
// side: 3 GB of L2 reads per launch at 1000 classes x 32 images x K = 24 (243 + 337 us).  Here the pairings are what they
// are -- K small GEMMs, one per prompt index i -- on the fp32 matrix pipe (v_mfma_f32_32x32x2_f32: exact fp32 products, fp32
// accumulation in a fixed order), every feature element read once per launch:
//   head_pairs:   P[i][b][c] = <x_bi, t_ci> / (|x_bi| |t_ci|); one wave per (32-class tile, i); leaves 1/|x|, 1/|t| in ni / nt
//   head_sum:     logits[b][c] = (scale / K) sum_i P[i][b][c]                           (fixed order)
//   head_ce_kernel (above), also writing dl transposed
//   head_rowdots: s_t[c,i] = sum_b dl[b,c] P[i][b][c],  s_x[b,i] = sum_c dl[b,c] P[i][b][c]   (= <h, dh> of the row)
//   head_bwd_text / head_bwd_img:  df = (dh - h <h, dh>) / |f|,  dh = sum_o dl(g, o) other_hat[o, i, :]  as
//                 D[class][e] = sum_b (dl[b,c] / |x_bi|) x_bi[e]   resp.   D[b][e] = sum_c (dl[b,c] / |t_ci|) t_ci[e]
// Lane maps of the MFMA (probe_kernel below): operand values come from (row l31, k = half) of A and B; acc[r] is
// D[(r & 3) + 8 (r >> 2) + 4 half][l31].
__device__ __forceinline__ int mfma_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

template <bool PK>
__global__ __launch_bounds__(64) void head_pairs_kernel(const float* __restrict__ f_img, const float* __restrict__ f_txt,
                                                        float* ni, float* nt, float* part, int B, int C, int K, int e,
                                                        HeadGroups hg) {
  __shared__ float s_ix[32];
  {
    const int64_t s = blockIdx.z;
    f_img += s * hg.img; f_txt += s * hg.txt; ni += s * hg.ws; nt += s * hg.ws; part += s * hg.ws;
  }
  const int lane = threadIdx.x, l31 = lane & 31, half = lane >> 5;
  const int c0 = blockIdx.x * 32, i = blockIdx.y;
  if (PK && i >= head_k<PK>(hg, blockIdx.z, K)) return;                       // (nothing downstream reads P[i], ni, nt of such a pair)
  const int c = min(c0 + l31, C - 1);
  const float* t = f_txt + ((int64_t)c * K + i) * e + 4 * half;    // this lane's k's of an 8-wide step: 4 half .. 4 half + 3
  for (int b0 = 0; b0 < B; b0 += 32) {
    const int b = min(b0 + l31, B - 1);
    const float* x = f_img + ((int64_t)b * K + i) * e + 4 * half;
    f32x16_t d;
#pragma unroll
    for (int r = 0; r < 16; ++r) d[r] = 0.f;
    float st = 0.f, sx = 0.f;
    for (int q0 = 0; q0 < e; q0 += 32) {                            // (e % 32 == 0: the launcher) 8 loads in flight, 16 MFMAs
      float4 xv[4], tv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        xv[j] = *reinterpret_cast<const float4*>(x + q0 + 8 * j);
        tv[j] = *reinterpret_cast<const float4*>(t + q0 + 8 * j);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        d = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[j].x, tv[j].x, d, 0, 0, 0);
        d = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[j].y, tv[j].y, d, 0, 0, 0);
        d = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[j].z, tv[j].z, d, 0, 0, 0);
        d = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[j].w, tv[j].w, d, 0, 0, 0);
        sx = fmaf(xv[j].x, xv[j].x, sx); sx = fmaf(xv[j].y, xv[j].y, sx); sx = fmaf(xv[j].z, xv[j].z, sx); sx = fmaf(xv[j].w, xv[j].w, sx);
        st = fmaf(tv[j].x, tv[j].x, st); st = fmaf(tv[j].y, tv[j].y, st); st = fmaf(tv[j].z, tv[j].z, st); st = fmaf(tv[j].w, tv[j].w, st);
      }
    }
    sx += __shfl_xor(sx, 32);                                       // the two halves of the row
    st += __shfl_xor(st, 32);
    const float ix = 1.0f / sqrtf(sx), it = 1.0f / sqrtf(st);
    __syncthreads();                                                // (the previous image tile's readers are done)
    if (half == 0) {
      s_ix[l31] = ix;
      if (blockIdx.x == 0 && b0 + l31 < B) ni[(int64_t)b * K + i] = ix;
      if (b0 == 0 && c0 + l31 < C) nt[(int64_t)c * K + i] = it;
    }
    __syncthreads();
    if (c0 + l31 < C) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int bb = b0 + mfma_row(r, half);
        if (bb < B) part[((int64_t)i * B + bb) * C + c] = d[r] * s_ix[mfma_row(r, half)] * it;
      }
    }
  }
}

template <bool PK>
__global__ __launch_bounds__(256) void head_sum_kernel(const float* __restrict__ part, float* logits, int BC, int K, float mul,
                                                      HeadGroups hg) {
  part += (int64_t)blockIdx.y * hg.ws; logits += (int64_t)blockIdx.y * hg.bc;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= BC) return;
  const int ku = head_k<PK>(hg, blockIdx.y, K);
  float s = 0.f;
  for (int i = 0; i < ku; ++i) s += part[(int64_t)i * BC + idx];
  logits[idx] = s * head_mul<PK>(hg, ku, mul);
}

// blocks [0, K * ceil(C / 256)): s_t, one thread per (i, c); then B * K blocks: s_x, one block per (b, i); block 0 also the
// mean loss
template <bool PK>
__global__ __launch_bounds__(256) void head_rowdots_kernel(const float* __restrict__ dl, const float* __restrict__ part,
                                                           float* s_t, float* s_x, int B, int C, int K,
                                                           const float* loss_b, float* loss, HeadGroups hg) {
  __shared__ float red[4];
  {
    const int64_t s = blockIdx.y;
    dl += s * hg.ws; part += s * hg.ws; s_t += s * hg.ws; s_x += s * hg.ws; loss_b += s * hg.ws; loss = head_shift(loss, s);
  }
  const int ct = (C + 255) / 256;
  if (loss != nullptr && blockIdx.x == 0 && threadIdx.x == 0) {    // mean CE over the batch, fixed summation order
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += loss_b[b];
    *loss = s / (float)B;
  }
  const int ku = head_k<PK>(hg, blockIdx.y, K);
  if ((int)blockIdx.x < K * ct) {
    const int i = blockIdx.x / ct, c = (blockIdx.x - i * ct) * 256 + threadIdx.x;
    if (c >= C || (PK && i >= ku)) return;
    float s = 0.f;
    for (int b = 0; b < B; ++b) s = fmaf(dl[(int64_t)b * C + c], part[((int64_t)i * B + b) * C + c], s);
    s_t[(int64_t)c * K + i] = s;
  } else {
    const int row = blockIdx.x - K * ct, b = row / K, i = row - b * K;
    if (PK && i >= ku) return;
    float s = 0.f;
    for (int c = threadIdx.x; c < C; c += 256) s = fmaf(dl[(int64_t)b * C + c], part[((int64_t)i * B + b) * C + c], s);
    s = block_sum(s, red);
    if (threadIdx.x == 0) s_x[row] = s;
  }
}

// d text_f: one wave per (32-class tile, i, group of e-tiles); D[class][e] over the image pairs (2 kk, 2 kk + 1)
template <bool PK>
__global__ __launch_bounds__(64) void head_bwd_text_kernel(const float* __restrict__ dl, const float* __restrict__ f_img,
                                                           const float* __restrict__ ni, const float* __restrict__ f_txt,
                                                           const float* __restrict__ nt, const float* __restrict__ s_t,
                                                           float* d_text_f, void* d_text_a, int act_dtype, int B, int C,
                                                           int K, int e, int etiles_per_block, int ez,
                                                           HeadGroups hg) {
  const int lane = threadIdx.x, l31 = lane & 31, half = lane >> 5;
  const int bz = blockIdx.z % ez;                                   // blockIdx.z = group * ez + e-tile group
  {
    const int64_t s = blockIdx.z / ez;
    dl += s * hg.ws; ni += s * hg.ws; nt += s * hg.ws; s_t += s * hg.ws;
    f_img += s * hg.img; f_txt += s * hg.txt; d_text_f += s * hg.txt; d_text_a = head_shift16(d_text_a, s * hg.txt);
  }
  const int c0 = blockIdx.x * 32, i = blockIdx.y;
  const int ku = head_k<PK>(hg, blockIdx.z / ez, K);
  if (PK && i >= ku) {                                              // a pair this group does not use: zeros, nothing read
    for (int et = bz * etiles_per_block; et < min((bz + 1) * etiles_per_block, e >> 5); ++et)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int cn = c0 + mfma_row(r, half);
        if (cn < C) head_store(d_text_f, d_text_a, act_dtype, ((int64_t)cn * K + i) * e + et * 32 + l31, head_fill(ku));
      }
    return;
  }
  const int c = min(c0 + l31, C - 1);
  float itv[16], cf[16];                                            // per accumulator row: 1 / |t|, <h, dh> / |t|^2
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int cn = min(c0 + mfma_row(r, half), C - 1);
    const float it = nt[(int64_t)cn * K + i];
    itv[r] = it; cf[r] = it * it * s_t[(int64_t)cn * K + i];
  }
  const int npair = (B + 1) >> 1;
  // weights of 16 image pairs at a time (pairs past B: weight 0); one chunk (B <= 32): formed once for all e-tiles
  auto weights = [&](int kk0, float (&a)[16]) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int b = 2 * (kk0 + j) + half, bc = min(b, B - 1);
      a[j] = dl[(int64_t)bc * C + c] * ni[(int64_t)bc * K + i];
      if (b >= B) a[j] = 0.f;
    }
  };
  float a0[16];
  weights(0, a0);
  for (int et = bz * etiles_per_block; et < min((bz + 1) * etiles_per_block, e >> 5); ++et) {
    const int col = et * 32 + l31;
    f32x16_t d;
    float tq[16], xv[16];                                           // the rows' own values (epilogue), requested up front
#pragma unroll
    for (int j = 0; j < 16; ++j) xv[j] = f_img[((int64_t)min(2 * j + half, B - 1) * K + i) * e + col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      d[r] = 0.f;
      tq[r] = f_txt[((int64_t)min(c0 + mfma_row(r, half), C - 1) * K + i) * e + col];
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) d = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], xv[j], d, 0, 0, 0);
    for (int kk0 = 16; kk0 < npair; kk0 += 16) {                    // more than 32 images
      float a[16];
      weights(kk0, a);
#pragma unroll
      for (int j = 0; j < 16; ++j) xv[j] = f_img[((int64_t)min(2 * (kk0 + j) + half, B - 1) * K + i) * e + col];
#pragma unroll
      for (int j = 0; j < 16; ++j) d = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], xv[j], d, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int cn = c0 + mfma_row(r, half);
      if (cn < C) {
        const int64_t off = ((int64_t)cn * K + i) * e + col;
        head_store(d_text_f, d_text_a, act_dtype, off, d[r] * itv[r] - tq[r] * cf[r]);
      }
    }
  }
}

// d img_f: one workgroup per (i, e-tile, 32-image tile); D[image][e] over the class pairs, which the 8 waves split (wave w:
// pairs w, w + 8, ... in batches of 8: 24 loads in flight per wave, ~3 waves per SIMD at 1000 classes); the eight partial
// tiles are summed through LDS in wave order.  dlT = dl transposed [C][B].
constexpr int HEAD_IMG_WAVES = 8;
template <bool PK>
__global__ __launch_bounds__(64 * HEAD_IMG_WAVES) void head_bwd_img_kernel(
    const float* __restrict__ dlT, const float* __restrict__ f_img, const float* __restrict__ ni,
    const float* __restrict__ f_txt, const float* __restrict__ nt, const float* __restrict__ s_x, float* d_img_f,
    void* d_img_a, int act_dtype, int B, int C, int K, int e, int btiles, HeadGroups hg) {
  __shared__ float s_part[HEAD_IMG_WAVES][16][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, half = lane >> 5;
  {
    const int64_t s = blockIdx.z / btiles;                          // blockIdx.z = group * btiles + 32-image tile
    dlT += s * hg.ws; ni += s * hg.ws; nt += s * hg.ws; s_x += s * hg.ws;
    f_img += s * hg.img; f_txt += s * hg.txt; d_img_f += s * hg.img; d_img_a = head_shift16(d_img_a, s * hg.img);
  }
  const int i = blockIdx.x, col = blockIdx.y * 32 + l31, b0 = (blockIdx.z % btiles) * 32;
  const int ku = head_k<PK>(hg, blockIdx.z / btiles, K);
  if (PK && i >= ku) {                                              // a pair this group does not use: zeros, nothing read
#pragma unroll
    for (int rr = 0; rr < 16 / HEAD_IMG_WAVES; ++rr) {
      const int bn = b0 + mfma_row(wave + HEAD_IMG_WAVES * rr, half);
      if (bn < B) head_store(d_img_f, d_img_a, act_dtype, ((int64_t)bn * K + i) * e + col, head_fill(ku));
    }
    return;
  }
  const int b = min(b0 + l31, B - 1);
  f32x16_t d;
#pragma unroll
  for (int r = 0; r < 16; ++r) d[r] = 0.f;
  const int npair = (C + 1) >> 1;
  for (int kk0 = wave; kk0 < npair; kk0 += 8 * HEAD_IMG_WAVES) {   // (pairs past C: weight 0)
    float a[8], tv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int cc = 2 * (kk0 + j * HEAD_IMG_WAVES) + half, ccl = min(cc, C - 1);
      a[j] = dlT[(int64_t)ccl * B + b] * nt[(int64_t)ccl * K + i];
      if (cc >= C) a[j] = 0.f;
      tv[j] = f_txt[((int64_t)ccl * K + i) * e + col];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) d = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], tv[j], d, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) s_part[wave][r][lane] = d[r];
  __syncthreads();
#pragma unroll
  for (int rr = 0; rr < 16 / HEAD_IMG_WAVES; ++rr) {
    const int r = wave + HEAD_IMG_WAVES * rr;
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < HEAD_IMG_WAVES; ++w) v += s_part[w][r][lane];
    const int bn = b0 + mfma_row(r, half);
    if (bn < B) {
      const float ix = ni[(int64_t)bn * K + i];
      const int64_t off = ((int64_t)bn * K + i) * e + col;
      head_store(d_img_f, d_img_a, act_dtype, off, v * ix - f_img[off] * (ix * ix * s_x[(int64_t)bn * K + i]));
    }
  }
}

// ---- MFMA layout probe ------------------------------------------------------------------------
// ---- empirical peaks ("measure empirical peaks on the box ... and use those as denominators too") ----
// pure-MFMA loop: every wave keeps 4 independent 32x32 accumulators busy, nothing else.  which: 0 bf16, 1 f32.
template <int WHICH>
__global__ __launch_bounds__(256) void peak_mfma_kernel(float* sink, int iters) {
  f32x16_t acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  // random-looking, non-zero operands: zero-filled operands run faster than real data on this chip
  // WHICH == 2: the same bf16 loop on ZERO operands -- the chip clocks to its power budget, so zero operands run at
  // ~2.4 GHz and random ones at ~1.65-1.9 GHz (guide: DVFS give-back); the two readings bracket what "peak" means here
  const float seed = WHICH == 2 ? 0.0f : 0.001f * (float)((threadIdx.x * 37 + blockIdx.x * 11) % 251) - 0.125f;
  if constexpr (WHICH == 0 || WHICH == 2) {
    bf16x8_t a, b;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      a[i] = (__bf16)(WHICH == 2 ? 0.0f : seed + 0.01f * i);
      b[i] = (__bf16)(WHICH == 2 ? 0.0f : 0.5f - seed * (i + 1));
    }
    for (int it = 0; it < iters; ++it) {
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[t], 0, 0, 0);
    }
  } else {
    float a = seed, b = 0.5f - seed;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[t], 0, 0, 0);
    }
  }
  float s = 0.f;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) s += acc[t][r];
  if (s == 12345.678f) sink[0] = s;           // keeps the loop alive; practically never true
}

__global__ __launch_bounds__(256) void peak_copy_kernel(const uint4* __restrict__ src, uint4* dst, int64_t n16) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride) dst[i] = src[i];
}

__global__ void probe_kernel(int which, const float* a, const float* b, float* d) {
  const int lane = threadIdx.x & 63, half = lane >> 5, l31 = lane & 31;
  f32x16_t acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  if (which == 0) {
    float fa[8], fb[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { fa[j] = a[l31 * 16 + half * 8 + j]; fb[j] = b[l31 * 16 + half * 8 + j]; }
    typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
    u32x4 ua, ub;
#pragma unroll
    for (int j = 0; j < 4; ++j) { ua[j] = pack_bf16x2(fa[2 * j], fa[2 * j + 1]); ub[j] = pack_bf16x2(fb[2 * j], fb[2 * j + 1]); }
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, ua), __builtin_bit_cast(bf16x8_t, ub), acc, 0, 0, 0);
  } else {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[l31 * 2 + half], b[l31 * 2 + half], acc, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = (r & 3) + 8 * (r >> 2) + 4 * half;   // row: from operand A
    d[i * 32 + l31] = acc[r];                           // col: from operand B
  }
}

}  // namespace

extern "C" int rpo_version(void) { return RPO_ABI_VERSION; }

extern "C" const char* rpo_error_string(int code) {
  switch (code) {
    case 0: return "ok";
    case RPO_E_BADARG: return "rpo: null pointer or non-positive size";
    case RPO_E_SHAPE: return "rpo: shape not supported by the kernel";
    case RPO_E_DTYPE: return "rpo: dtype combination not supported";
    case RPO_E_ALIGN: return "rpo: pointer or leading dimension not sufficiently aligned";
    case RPO_E_WORKSPACE: return "rpo: workspace or table bound too small for this call";
    case RPO_E_JPEG_CORRUPT: return "rpo: jpeg: not a JPEG file, or a truncated / inconsistent header";
    case RPO_E_JPEG_PROGRESSIVE: return "rpo: jpeg: progressive frame (decode on the host)";
    case RPO_E_JPEG_ARITHMETIC: return "rpo: jpeg: arithmetic coding (decode on the host)";
    case RPO_E_JPEG_LOSSLESS: return "rpo: jpeg: lossless or hierarchical frame (decode on the host)";
    case RPO_E_JPEG_PRECISION: return "rpo: jpeg: 12-bit samples or 16-bit quantisation tables (decode on the host)";
    case RPO_E_JPEG_COMPONENTS: return "rpo: jpeg: neither 1 nor 3 components, e.g. CMYK (decode on the host)";
    case RPO_E_JPEG_RGB: return "rpo: jpeg: RGB-coded file, no YCbCr transform (decode on the host)";
    case RPO_E_JPEG_SAMPLING: return "rpo: jpeg: chroma sampling other than 4:4:4 / 4:2:2 / 4:2:0 (decode on the host)";
    case RPO_E_JPEG_MULTISCAN: return "rpo: jpeg: components spread over several scans (decode on the host)";
    case RPO_E_JPEG_SCRIPT: return "rpo: jpeg: progressive scan script incomplete or inconsistent (decode on the host)";
    case RPO_E_JPEG_SEQUENTIAL: return "rpo: jpeg: a sequential frame: rpo_jpeg_probe handles it, not rpo_jpeg_prog_probe";
    default: return code > 0 ? hipGetErrorString((hipError_t)code) : "rpo: unknown error";
  }
}

extern "C" int rpo_im2col_patches(const float* img, void* out, int out_dtype, int64_t ldo, int B, int H, int W,
                                  int patch, void* stream) {
  if (!img || !out || B <= 0 || H <= 0 || W <= 0 || patch <= 0) return RPO_E_BADARG;
  if (H % patch || W % patch || patch % 2 || ldo < 3 * patch * patch) return RPO_E_SHAPE;
  if (reinterpret_cast<uintptr_t>(img) % 8) return RPO_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int esz = out_dtype == RPO_F32 ? 4 : 2;
  if (patch % 8 == 0 && reinterpret_cast<uintptr_t>(img) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0 &&
      (ldo * esz) % 16 == 0) {
    const int64_t total8 = (int64_t)B * 3 * H * (W / 8);
    const unsigned blocks8 = (unsigned)((total8 + 255) / 256);
    if (out_dtype == RPO_BF16)
      hipLaunchKernelGGL(im2col8_kernel<bf16_t>, dim3(blocks8), dim3(256), 0, s, img,
                         static_cast<bf16_t*>(out), ldo, B, H, W, patch, total8);
    else if (out_dtype == RPO_F16)
      hipLaunchKernelGGL(im2col8_kernel<f16_t>, dim3(blocks8), dim3(256), 0, s, img,
                         static_cast<f16_t*>(out), ldo, B, H, W, patch, total8);
    else if (out_dtype == RPO_F32)
      hipLaunchKernelGGL(im2col8_kernel<float>, dim3(blocks8), dim3(256), 0, s, img,
                         static_cast<float*>(out), ldo, B, H, W, patch, total8);
    else return RPO_E_DTYPE;
    return rpo_launch_status();
  }
  const int64_t total = (int64_t)B * 3 * H * (W / 2);
  const unsigned blocks = (unsigned)((total + 255) / 256);
  if (out_dtype == RPO_BF16)
    hipLaunchKernelGGL(im2col_kernel<bf16_t>, dim3(blocks), dim3(256), 0, s, img,
                       static_cast<bf16_t*>(out), ldo, B, H, W, patch, total);
  else if (out_dtype == RPO_F16)
    hipLaunchKernelGGL(im2col_kernel<f16_t>, dim3(blocks), dim3(256), 0, s, img,
                       static_cast<f16_t*>(out), ldo, B, H, W, patch, total);
  else if (out_dtype == RPO_F32)
    hipLaunchKernelGGL(im2col_kernel<float>, dim3(blocks), dim3(256), 0, s, img,
                       static_cast<float*>(out), ldo, B, H, W, patch, total);
  else return RPO_E_DTYPE;
  return rpo_launch_status();
}

extern "C" int rpo_img_assemble(float* x, int64_t ldx, const float* cls, const float* pos0,
                                const float* img_prompt, int B, int N, int Kp, int d, void* stream) {
  if (!x || !cls || !pos0 || B <= 0 || N <= 0 || Kp < 0 || d <= 0 || (Kp > 0 && !img_prompt)) return RPO_E_BADARG;
  hipLaunchKernelGGL(assemble_kernel, dim3(B + B * Kp), dim3(256), 0, static_cast<hipStream_t>(stream), x, ldx,
                     cls, pos0, img_prompt, B, N, Kp, d);
  return rpo_launch_status();
}

extern "C" int rpo_broadcast_rows(const float* src, float* dst, int64_t ld, int groups, int rows, int d,
                                  void* stream) {
  return rpo_broadcast_rows_sets(src, (int64_t)rows * d, dst, ld, 1, groups, rows, d, stream);
}

extern "C" int rpo_broadcast_rows_sets(const float* src, int64_t src_set_stride, float* dst, int64_t ld, int sets,
                                       int groups, int rows, int d, void* stream) {
  if (!src || !dst || sets <= 0 || groups <= 0 || rows <= 0 || d <= 0 || src_set_stride < 0) return RPO_E_BADARG;
  if ((int64_t)sets * groups * rows >= (1ll << 31)) return RPO_E_SHAPE;
  hipLaunchKernelGGL(broadcast_rows_kernel, dim3(sets * groups * rows), dim3(256), 0, static_cast<hipStream_t>(stream),
                     src, dst, ld, rows, d, groups * rows, src_set_stride);
  return rpo_launch_status();
}

extern "C" int rpo_text_embed(const int32_t* ids, int64_t ld_ids, const float* table, int vocab, const float* pos,
                              const float* ctx, int n_ctx, float* out, int n, int L, int d, void* stream) {
  if (!ids || !table || !pos || !out || n < 1 || L < 1 || vocab < 1 || n_ctx < 0 || (n_ctx > 0 && !ctx)) return RPO_E_BADARG;
  if (d < 4 || d % 4 != 0 || L > ld_ids) return RPO_E_SHAPE;
  if (!aligned16(table) || !aligned16(pos) || !aligned16(out) || (n_ctx > 0 && !aligned16(ctx))) return RPO_E_ALIGN;
  const int64_t rows = (int64_t)n * L;
  const int grid = (int)(rows < 4096 ? rows : 4096);            // 16 workgroups of two waves per CU, then the stride loop
  hipLaunchKernelGGL(text_embed_kernel, dim3(grid), dim3(128), 0, static_cast<hipStream_t>(stream), ids, ld_ids,
                     reinterpret_cast<const float4*>(table), vocab, reinterpret_cast<const float4*>(pos),
                     reinterpret_cast<const float4*>(n_ctx > 0 ? ctx : nullptr), n_ctx, reinterpret_cast<float4*>(out), rows, L,
                     d / 4);
  return rpo_launch_status();
}

extern "C" int rpo_reduce_groups(const float* src, int64_t ld, float* out, int groups, int rows, int d,
                                 void* stream) {
  return rpo_reduce_groups_sets(src, ld, out, (int64_t)rows * d, 1, groups, rows, d, stream);
}

extern "C" int rpo_reduce_groups_sets(const float* src, int64_t ld, float* out, int64_t out_set_stride, int sets,
                                      int groups, int rows, int d, void* stream) {
  if (!src || !out || sets <= 0 || groups <= 0 || rows <= 0 || d <= 0) return RPO_E_BADARG;
  if (sets > 1 && out_set_stride < (int64_t)rows * d) return RPO_E_SHAPE;
  if (sets > 65535) return RPO_E_SHAPE;
  if (groups >= 64)          // (below: the one-thread-per-element kernel, whose order the Oxford-Pets goldens were validated with)
    hipLaunchKernelGGL(reduce_groups_wide_kernel, dim3(rows * ((d + 31) / 32), sets), dim3(256), 0,
                       static_cast<hipStream_t>(stream), src, ld, out, groups, rows, d, out_set_stride);
  else
    hipLaunchKernelGGL(reduce_groups_kernel, dim3((rows * d + 255) / 256, sets), dim3(256), 0,
                       static_cast<hipStream_t>(stream), src, ld, out, groups, rows, d, out_set_stride);
  return rpo_launch_status();
}

extern "C" int64_t rpo_head_workspace_floats(int B, int C, int K, int e) {
  return (int64_t)(B + C) * K * e + (int64_t)(B + C) * K + (int64_t)B * C + B;
}

// S independent heads (S = 1: the plain call); group s works in workspace [s * wsg, (s + 1) * wsg), wsg =
// rpo_head_workspace_floats(B, C, K, e), laid out as a single head's.
template <bool PK>
static int head_impl(const float* img_f, const float* text_f, const int64_t* label, float scale_exp, float* logits,
                     float* loss, float* d_img_f, float* d_text_f, void* d_img_act, void* d_text_act, int act_dtype, int S,
                     int B, int C, int K, int e, float* ws, void* stream, const int32_t* k_used = nullptr) {
  if (PK != (k_used != nullptr)) return RPO_E_BADARG;
  if (!img_f || !text_f || !logits || !ws || S <= 0 || B <= 0 || C <= 0 || K <= 0 || e <= 0) return RPO_E_BADARG;
  if ((d_img_act || d_text_act) && act_dtype != RPO_BF16 && act_dtype != RPO_F16) return RPO_E_DTYPE;
  if (label && (!loss || !d_img_f || !d_text_f)) return RPO_E_BADARG;
  if (e > 1024 || S > 1024 || (int64_t)((B + 31) / 32) * S > 65535) return RPO_E_SHAPE;   // (grid.z of the image backward)
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint32_t G = (uint32_t)S;
  const HeadGroups hg{(int64_t)B * K * e, (int64_t)C * K * e, (int64_t)B * C, (int64_t)B, rpo_head_workspace_floats(B, C, K, e),
                      k_used, scale_exp};
  float* ni = ws;
  float* nt = ni + (int64_t)B * K;
  float* dl = nt + (int64_t)C * K;
  float* lb = dl + (int64_t)B * C;
  const float gmul = scale_exp / ((float)K * (float)B);
  const float mul = scale_exp / (float)K;
  // Large class sets on the fp32 matrix pipe (kernels above).  Their scratch -- P [K][B][C], dl transposed, s_t, s_x -- lies
  // in the workspace behind the arrays of the small-set path; sets whose scratch does not fit keep the kernels above.
  float* part = lb + B;
  float* dlT = part + (int64_t)K * B * C;
  float* s_t = dlT + (int64_t)B * C;
  float* s_x = s_t + (int64_t)C * K;
#ifdef RPO_HEAD_NO_MFMA
  const bool mfma_head = false;
#else
  const bool mfma_head = C > 128 && e % 32 == 0 && aligned16(img_f) && aligned16(text_f) &&
                         (s_x + (int64_t)B * K) - ws <= rpo_head_workspace_floats(B, C, K, e) && (int64_t)B * C < (1ll << 31);
#endif
  if (mfma_head) {
    hipLaunchKernelGGL(head_pairs_kernel<PK>, dim3((C + 31) / 32, K, G), dim3(64), 0, s, img_f, text_f, ni, nt, part, B, C, K, e, hg);
    hipLaunchKernelGGL(head_sum_kernel<PK>, dim3((B * C + 255) / 256, G), dim3(256), 0, s, part, logits, B * C, K, mul, hg);
    if (!label) return rpo_launch_status();
    hipLaunchKernelGGL(head_ce_kernel<PK>, dim3(B, G), dim3(256), 0, s, logits, label, dl, lb, C, gmul, dlT, B, hg);
    hipLaunchKernelGGL(head_rowdots_kernel<PK>, dim3(K * ((C + 255) / 256) + B * K, G), dim3(256), 0, s, dl, part, s_t, s_x, B, C, K,
                       lb, loss, hg);
#ifndef RPO_HEAD_TEXT_EZ
#define RPO_HEAD_TEXT_EZ 4
#endif
    const int etiles = e / 32, ez = etiles >= RPO_HEAD_TEXT_EZ ? RPO_HEAD_TEXT_EZ : 1;
    const int btiles = (B + 31) / 32;
    hipLaunchKernelGGL(head_bwd_text_kernel<PK>, dim3((C + 31) / 32, K, ez * G), dim3(64), 0, s, dl, img_f, ni, text_f, nt, s_t,
                       d_text_f, d_text_act, act_dtype, B, C, K, e, (etiles + ez - 1) / ez, ez, hg);
    hipLaunchKernelGGL(head_bwd_img_kernel<PK>, dim3(K, etiles, btiles * G), dim3(64 * HEAD_IMG_WAVES), 0, s, dlT, img_f, ni, text_f, nt, s_x,
                       d_img_f, d_img_act, act_dtype, B, C, K, e, btiles, hg);
    return rpo_launch_status();
  }
  if (B > 65535) return RPO_E_SHAPE;
  if (e % 256 == 0 && aligned16(img_f) && aligned16(text_f))
    hipLaunchKernelGGL((head_logits_kernel<true, PK>), dim3(C, B, G), dim3(256), 0, s, img_f, text_f, ni, nt, logits, C, K, e, mul, hg);
  else
    hipLaunchKernelGGL((head_logits_kernel<false, PK>), dim3(C, B, G), dim3(256), 0, s, img_f, text_f, ni, nt, logits, C, K, e, mul, hg);
  if (!label) return rpo_launch_status();
  // Small class sets (the few-shot base / new splits; 19 for Oxford-Pets base): two launches per training step, the
  // cross-entropy is recomputed inside the backward blocks.  Larger ones (ImageNet: 500 / 1000 classes) get their own
  // cross-entropy launch and a dl array.
  const int nmax = B > C ? B : C;
  if (C <= 128 && B <= 2048) {
    hipLaunchKernelGGL((head_bwd_kernel<true, PK>), dim3(B * K + C * K, G), dim3(256), (size_t)(nmax + 3 * B) * sizeof(float), s,
                       dl, img_f, ni, text_f, nt, d_img_f, d_text_f, B, C, K, e, lb, loss, logits, label, gmul, d_img_act, d_text_act, act_dtype, hg);
    return rpo_launch_status();
  }
  if ((size_t)nmax * sizeof(float) > 64 * 1024) return RPO_E_SHAPE;
  hipLaunchKernelGGL(head_ce_kernel<PK>, dim3(B, G), dim3(256), 0, s, logits, label, dl, lb, C, gmul, static_cast<float*>(nullptr), 0, hg);
  hipLaunchKernelGGL((head_bwd_kernel<false, PK>), dim3(B * K + C * K, G), dim3(256), (size_t)nmax * sizeof(float), s, dl, img_f,
                     ni, text_f, nt, d_img_f, d_text_f, B, C, K, e, lb, loss, logits, label, gmul, d_img_act, d_text_act, act_dtype, hg);
  return rpo_launch_status();
}

extern "C" int rpo_head_fwd_bwd(const float* img_f, const float* text_f, const int64_t* label, float scale_exp,
                                float* logits, float* loss, float* d_img_f, float* d_text_f, int B, int C, int K,
                                int e, float* ws, void* stream) {
  return head_impl<false>(img_f, text_f, label, scale_exp, logits, loss, d_img_f, d_text_f, nullptr, nullptr, RPO_F32, 1, B, C, K, e,
                   ws, stream);
}

extern "C" int rpo_head_fwd_bwd_act(const float* img_f, const float* text_f, const int64_t* label, float scale_exp,
                                    float* logits, float* loss, float* d_img_f, float* d_text_f, void* d_img_act,
                                    void* d_text_act, int act_dtype, int B, int C, int K, int e, float* ws,
                                    void* stream) {
  return head_impl<false>(img_f, text_f, label, scale_exp, logits, loss, d_img_f, d_text_f, d_img_act, d_text_act, act_dtype, 1, B,
                   C, K, e, ws, stream);
}

extern "C" int rpo_head_fwd_bwd_grouped(const float* img_f, const float* text_f, const int64_t* label, float scale_exp,
                                        float* logits, float* loss, float* d_img_f, float* d_text_f, int S, int B, int C,
                                        int K, int e, float* ws, void* stream) {
  return head_impl<false>(img_f, text_f, label, scale_exp, logits, loss, d_img_f, d_text_f, nullptr, nullptr, RPO_F32, S, B, C, K, e,
                   ws, stream);
}

extern "C" int rpo_head_fwd_bwd_grouped_act(const float* img_f, const float* text_f, const int64_t* label,
                                            float scale_exp, float* logits, float* loss, float* d_img_f, float* d_text_f,
                                            void* d_img_act, void* d_text_act, int act_dtype, int S, int B, int C, int K,
                                            int e, float* ws, void* stream) {
  return head_impl<false>(img_f, text_f, label, scale_exp, logits, loss, d_img_f, d_text_f, d_img_act, d_text_act, act_dtype, S,
                          B, C, K, e, ws, stream);
}

// Per-group K: the grouped head with k_used[s] of the K pairs in use in group s (HeadGroups::k).  The same kernels and
// launches, in their PK instances; callers without per-group K keep the entry points above and the instances they had.
extern "C" int rpo_head_fwd_bwd_grouped_k(const float* img_f, const float* text_f, const int64_t* label, float scale_exp,
                                          float* logits, float* loss, float* d_img_f, float* d_text_f, void* d_img_act,
                                          void* d_text_act, int act_dtype, int S, int B, int C, int K, int e,
                                          const int32_t* k_used, float* ws, void* stream) {
  if (!k_used) return RPO_E_BADARG;
  return head_impl<true>(img_f, text_f, label, scale_exp, logits, loss, d_img_f, d_text_f, d_img_act, d_text_act, act_dtype, S, B,
                         C, K, e, ws, stream, k_used);
}

// ---- CoCoOp's meta-net (trainers/cocoop.py:93-97, :137-143) -----------------------------------------------------------
// bias[b] = linear2(relu(linear1(f[b] / |f[b]|))): vis_dim -> vis_dim / 16 -> ctx_dim, one workgroup per image; the
// normalised feature and the hidden activation are kept for the backward.  fp32 throughout (the reference's fp16 branch
// halves the meta-net; fp32 is its PREC = fp32 / amp behaviour).
namespace {
__global__ __launch_bounds__(256) void metanet_fwd_kernel(const float* __restrict__ f, const float* __restrict__ w1,
                                                          const float* __restrict__ b1, const float* __restrict__ w2,
                                                          const float* __restrict__ b2, float* fn, float* hid,
                                                          float* bias, int e, int h, int d) {
  extern __shared__ float mn_smem[];               // fn [e] | hid [h]
  __shared__ float red[4];
  float* sf = mn_smem;
  float* sh = mn_smem + e;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float ss = 0.f;
  for (int i = tid; i < e; i += 256) { const float v = f[(int64_t)b * e + i]; ss = fmaf(v, v, ss); }
  ss = block_sum(ss, red);
  const float inv = 1.0f / sqrtf(ss);
  for (int i = tid; i < e; i += 256) {
    const float v = f[(int64_t)b * e + i] * inv;
    sf[i] = v;
    fn[(int64_t)b * e + i] = v;
  }
  __syncthreads();
  for (int j = wave; j < h; j += 4) {              // one wave per hidden unit: fixed-order lane partials + wave_sum
    float a = 0.f;
    for (int i = lane; i < e; i += 64) a = fmaf(w1[(int64_t)j * e + i], sf[i], a);
    a = wave_sum(a);
    if (lane == 0) {
      const float v = fmaxf(a + b1[j], 0.f);
      sh[j] = v;
      hid[(int64_t)b * h + j] = v;
    }
  }
  __syncthreads();
  for (int o = tid; o < d; o += 256) {
    float a = b2[o];
    for (int j = 0; j < h; ++j) a = fmaf(w2[(int64_t)o * h + j], sh[j], a);
    bias[(int64_t)b * d + o] = a;
  }
}

// Gradients of the four meta-net tensors given dbias [B, d] (sum over the batch in fixed order b = 0 .. B-1):
//   g_w2[o][j] = sum_b dbias[b][o] hid[b][j];  g_b2[o] = sum_b dbias[b][o];
//   dhid[b][j] = (hid[b][j] > 0) sum_o dbias[b][o] w2[o][j];  g_w1[j][i] = sum_b dhid[b][j] fn[b][i];  g_b1[j] = sum_b dhid[b][j]
// Every block recomputes dhid (B * h dot products of length d: a few thousand MACs) into LDS, then owns 256 outputs.
__global__ __launch_bounds__(256) void metanet_bwd_kernel(const float* __restrict__ dbias, const float* __restrict__ fn,
                                                          const float* __restrict__ hid, const float* __restrict__ w2,
                                                          float* g_w1, float* g_b1, float* g_w2, float* g_b2, int B, int e,
                                                          int h, int d) {
  extern __shared__ float mn_smem[];               // dhid [B][h]
  const int tid = threadIdx.x;
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
}  // namespace

extern "C" int rpo_metanet_fwd(const float* img_f, const float* w1, const float* b1, const float* w2, const float* b2,
                               float* f_norm, float* hidden, float* bias, int B, int e, int h, int d, void* stream) {
  if (!img_f || !w1 || !b1 || !w2 || !b2 || !f_norm || !hidden || !bias || B <= 0 || e <= 0 || h <= 0 || d <= 0)
    return RPO_E_BADARG;
  if ((e + h) * 4 > 48 * 1024) return RPO_E_SHAPE;
  hipLaunchKernelGGL(metanet_fwd_kernel, dim3(B), dim3(256), (e + h) * 4, static_cast<hipStream_t>(stream), img_f, w1,
                     b1, w2, b2, f_norm, hidden, bias, e, h, d);
  return rpo_launch_status();
}

extern "C" int rpo_metanet_bwd(const float* d_bias, const float* f_norm, const float* hidden, const float* w2,
                               float* g_w1, float* g_b1, float* g_w2, float* g_b2, int B, int e, int h, int d,
                               void* stream) {
  if (!d_bias || !f_norm || !hidden || !w2 || !g_w1 || !g_b1 || !g_w2 || !g_b2 || B <= 0 || e <= 0 || h <= 0 || d <= 0)
    return RPO_E_BADARG;
  if ((int64_t)B * h * 4 > 48 * 1024) return RPO_E_SHAPE;
  const int64_t n = (int64_t)d * h + (int64_t)h * e + d + h;
  hipLaunchKernelGGL(metanet_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), B * h * 4,
                     static_cast<hipStream_t>(stream), d_bias, f_norm, hidden, w2, g_w1, g_b1, g_w2, g_b2, B, e, h, d);
  return rpo_launch_status();
}

extern "C" int rpo_sgd_step(float* p, const float* g, float* buf, int64_t n, float lr, float momentum, float wd,
                            float grad_scale, int first_step, void* stream) {
  if (!p || !g || !buf || n <= 0) return RPO_E_BADARG;
  hipLaunchKernelGGL(sgd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), p, g, buf, n, lr, momentum, wd, grad_scale, first_step);
  return rpo_launch_status();
}

extern "C" int rpo_sgd_step_guarded(float* p, const float* g, float* buf, int64_t n, float lr, float momentum, float wd,
                                    float grad_scale, int first_step, int32_t* found_inf, void* stream) {
  if (!p || !g || !buf || !found_inf || n <= 0) return RPO_E_BADARG;
  hipLaunchKernelGGL(sgd_guarded_kernel, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream), p, g, buf, n, lr,
                     momentum, wd, grad_scale, first_step, found_inf);
  return rpo_launch_status();
}

extern "C" int rpo_sgd_step_sets(float* p, const float* g, float* buf, int64_t set_stride, int sets, const float* hyper,
                                 const int32_t* used, int64_t seg0, int64_t seg1, int first_step, int32_t* found_inf,
                                 void* stream) {
  if (!p || !g || !buf || !hyper || sets <= 0 || seg0 < 0 || seg1 < 0 || seg0 + seg1 <= 0) return RPO_E_BADARG;
  if (set_stride < seg0 + seg1 || sets > 65535) return RPO_E_SHAPE;
  if (found_inf)
    hipLaunchKernelGGL(sgd_sets_guarded_kernel, dim3(sets), dim3(1024), 0, static_cast<hipStream_t>(stream), p, g, buf,
                       set_stride, hyper, used, seg0, seg1, first_step, found_inf);
  else
    hipLaunchKernelGGL(sgd_sets_kernel, dim3((unsigned)((seg0 + seg1 + 255) / 256), sets), dim3(256), 0,
                       static_cast<hipStream_t>(stream), p, g, buf, set_stride, hyper, used, seg0, seg1, first_step);
  return rpo_launch_status();
}

extern "C" int rpo_convert(const float* src, int64_t lds, void* dst, int dst_dtype, int64_t ldd, int rows,
                           int cols, void* stream) {
  if (!src || !dst || rows <= 0 || cols <= 0) return RPO_E_BADARG;
  const int64_t n = (int64_t)rows * cols;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dst_dtype == RPO_BF16)
    hipLaunchKernelGGL(convert_kernel<bf16_t>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, lds,
                       static_cast<bf16_t*>(dst), ldd, rows, cols);
  else if (dst_dtype == RPO_F16)
    hipLaunchKernelGGL(convert_kernel<f16_t>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, lds,
                       static_cast<f16_t*>(dst), ldd, rows, cols);
  else if (dst_dtype == RPO_F32)
    hipLaunchKernelGGL(convert_kernel<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, lds,
                       static_cast<float*>(dst), ldd, rows, cols);
  else return RPO_E_DTYPE;
  return rpo_launch_status();
}

extern "C" int rpo_probe_mfma(int which, const float* a, const float* b, float* d, void* stream) {
  if (!a || !b || !d || (which != 0 && which != 1)) return RPO_E_BADARG;
  hipLaunchKernelGGL(probe_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), which, a, b, d);
  return rpo_launch_status();
}

extern "C" int rpo_probe_peak_mfma(int which, int blocks, int iters, float* sink, double* flops, void* stream) {
  if (!sink || !flops || blocks <= 0 || iters <= 0 || which < 0 || which > 2) return RPO_E_BADARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (which == 0) hipLaunchKernelGGL(peak_mfma_kernel<0>, dim3(blocks), dim3(256), 0, s, sink, iters);
  else if (which == 2) hipLaunchKernelGGL(peak_mfma_kernel<2>, dim3(blocks), dim3(256), 0, s, sink, iters);
  else hipLaunchKernelGGL(peak_mfma_kernel<1>, dim3(blocks), dim3(256), 0, s, sink, iters);
  const double per_mfma = which != 1 ? 2.0 * 32 * 32 * 16 : 2.0 * 32 * 32 * 2;
  *flops = per_mfma * 4.0 * (double)iters * 4.0 * (double)blocks;   // 4 accumulators, 4 waves per block
  return rpo_launch_status();
}

extern "C" int rpo_probe_peak_copy(const void* src, void* dst, int64_t bytes, void* stream) {
  if (!src || !dst || bytes <= 0 || bytes % 16) return RPO_E_BADARG;
  if (reinterpret_cast<uintptr_t>(src) % 16 || reinterpret_cast<uintptr_t>(dst) % 16) return RPO_E_ALIGN;
  hipLaunchKernelGGL(peak_copy_kernel, dim3(256 * 16), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const uint4*>(src), static_cast<uint4*>(dst), bytes / 16);
  return rpo_launch_status();
}
