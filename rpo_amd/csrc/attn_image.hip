// Read-only masked attention of the image tower (forward for all rows, backward for the
// prompt rows), MFMA on gfx950.
//
// Reference semantics: nn.MultiheadAttention with the additive mask of
// trainers/rpo.py:154-156 -- the last K *columns* are -inf for every query row, so every
// query (CLS, patches, prompts) reads exactly the N = 1 + patches frozen keys of its own
// image and nothing reads a prompt.  exp(-inf) = 0 exactly, so the prompt columns are
// skipped instead of computed-and-masked.
//
// One workgroup per (image, head).  K and V of the N frozen tokens are staged ONCE into
// LDS (N <= 288, head_dim 64: <= 78 KB in bf16, <= 150 KB in f32; above 288 keys the *_long kernels below walk them in
// chunks of 256 with the same per-tile arithmetic) and every wave takes a
// 32-query tile.  The score tile is computed transposed, S^T = K . Q^T, so that by the
// 32x32 C/D map (col = lane&31, row = (reg&3)+8*(reg>>2)+4*(lane>>5)) a lane holds ONE
// query's scores in registers: the softmax row-reduce is an in-register reduction plus a
// single cross-half exchange (shuffle by 32), no LDS.  P stays in registers: its
// register->key order is taken as the contraction order of the P.V MFMAs and V is read
// from LDS in that same order (any k-permutation applied to both operands cancels), so no
// lane movement is needed between softmax and P.V.
//
// bf16: v_mfma_f32_32x32x16_bf16; K rows padded to 144 B.  The P.V (and, in the backward, dS.K) MFMAs
//       contract over KEYS, i.e. need the row-major [key][d] operand transposed.  It is transposed on the
//       matrix core itself: D = M_tile . I (A = 32 rows of M exactly as they sit in memory, B = identity)
//       lands in the C/D layout "lane = d, registers = keys", which after bf16 packing IS the A-operand
//       fragment of M^T in this kernel's key order -- exact, no 2-byte LDS scatter, no bank conflicts.
//       The forward does it once per key tile (one wave each) and parks the fragments in LDS
//       fragment-major (lane-linear 16-B writes/reads); the backward keeps them in registers.
// f32 : v_mfma_f32_32x32x2_f32 (exact f32 fma chain); one float per lane per operand, so
//       K and V stay row-major [Npad][65].
#include "common.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;

template <typename T, int NT> struct AL {   // LDS layout, 16-bit storage (bf16 / f16)
  static constexpr int NPAD = NT * 32;
  static constexpr int KROW = 144;                 // bytes per K (or row-major V) row: 128 + 16 pad
  static constexpr int K_BYTES = NPAD * KROW;
  static constexpr int F_BYTES = NT * 4 * 1024;                  // V^T fragments: [NT][2 dt][2 g2][64 lanes][16 B]
  static constexpr int PART_BYTES = 4 * 16 * 64 * 16 + 4 * 64 * 4;  // backward cross-wave partials
  static constexpr int FWD_BYTES = K_BYTES + F_BYTES;            // Ks | Vfrag
  static constexpr int BWD_STAGE = 2 * K_BYTES;                  // Ks | Vs
  static constexpr int BWD_BYTES = BWD_STAGE > PART_BYTES ? BWD_STAGE : PART_BYTES;
};
template <int NT> struct AL<float, NT> {
  static constexpr int NPAD = NT * 32;
  static constexpr int ROWF = 65;                  // floats per row
  static constexpr int K_BYTES = NPAD * ROWF * 4;
  static constexpr int PART_BYTES = 4 * 16 * 64 * 16 + 4 * 64 * 4;
  static constexpr int FWD_BYTES = 2 * K_BYTES;    // Ks | Vs
  static constexpr int BWD_STAGE = 2 * K_BYTES;
  static constexpr int BWD_BYTES = BWD_STAGE > PART_BYTES ? BWD_STAGE : PART_BYTES;
};

template <typename T> __device__ __forceinline__ bf16x8_t pack8(const float* p) {
  typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
  u32x4 u;
  u[0] = pack2<T>(p[0], p[1]); u[1] = pack2<T>(p[2], p[3]);
  u[2] = pack2<T>(p[4], p[5]); u[3] = pack2<T>(p[6], p[7]);
  return __builtin_bit_cast(bf16x8_t, u);
}
__device__ __forceinline__ bf16x8_t join8(uint2 lo, uint2 hi) {
  typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
  u32x4 u;
  u[0] = lo.x; u[1] = lo.y; u[2] = hi.x; u[3] = hi.y;
  return __builtin_bit_cast(bf16x8_t, u);
}

// B-operand identity fragment for the k-step pair (ks2 = 0, 1) of a 32-wide d' tile: element jj of lane
// (j = l31, half) is I[k][j] with k = 16*ks2 + 8*half + jj
template <typename T> __device__ __forceinline__ bf16x8_t ident_frag(int ks2, int l31, int half) {
  typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
  u32x4 u;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int k0 = 16 * ks2 + 8 * half + 2 * w;
    u[w] = (k0 == l31 ? One16<T>::lo : 0u) | (k0 + 1 == l31 ? One16<T>::hi : 0u);
  }
  return __builtin_bit_cast(bf16x8_t, u);
}
// rows[4] = the four 16-element A fragments (d = 0..63) of 32 rows of a row-major matrix M; returns the
// A fragments of M^T for d' tile dt: out[g2] covers this kernel's key slots 8*g2 .. 8*g2+7
template <typename T>
__device__ __forceinline__ void transpose_tile(const bf16x8_t (&rows)[4], int dt, const bf16x8_t& i0,
                                               const bf16x8_t& i1, bf16x8_t (&out)[2]) {
  f32x16_t d;
#pragma unroll
  for (int r = 0; r < 16; ++r) d[r] = 0.f;
  d = mfma16<T>(rows[2 * dt], i0, d);
  d = mfma16<T>(rows[2 * dt + 1], i1, d);
  float f[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) f[r] = d[r];
  out[0] = pack8<T>(f);
  out[1] = pack8<T>(f + 8);
}

// ---- staging ---------------------------------------------------------------------------
// rows [0, N) of one (image, head) slice: src + key*ld (already offset to the head), 64 elements.
// All global loads of a pass are issued before the first LDS write (fully unrolled, static
// register indices): a load-use-per-iteration loop serialises one HBM round trip per iteration
// and was the dominant cost of these kernels.
template <int NT, int NTHREADS>
__device__ __forceinline__ void stage_rows_bf16(char* dst, const bf16_t* src, int64_t ld, int N, int tid) {
  constexpr int CHUNKS = NT * 32 * 8;
  constexpr int ITERS = (CHUNKS + NTHREADS - 1) / NTHREADS;
  uint4 v[ITERS];
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int id = tid + it * NTHREADS;
    const int key = id >> 3, c = id & 7;
    v[it] = make_uint4(0, 0, 0, 0);
    if (id < CHUNKS && key < N) v[it] = *reinterpret_cast<const uint4*>(src + (int64_t)key * ld + c * 8);
  }
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int id = tid + it * NTHREADS;
    const int key = id >> 3, c = id & 7;
    if (id < CHUNKS) *reinterpret_cast<uint4*>(dst + key * 144 + c * 16) = v[it];
  }
}
// K and V row-major staging with every global load of both matrices in flight before the first LDS write
template <int NT, int NTHREADS>
__device__ __forceinline__ void stage2_bf16(char* dk, char* dv, const bf16_t* sk, const bf16_t* sv, int64_t ld, int N,
                                            int tid) {
  constexpr int CHUNKS = NT * 32 * 8;
  constexpr int ITERS = (CHUNKS + NTHREADS - 1) / NTHREADS;
  uint4 a[ITERS], b[ITERS];
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int id = tid + it * NTHREADS;
    const int key = id >> 3, c = id & 7;
    a[it] = make_uint4(0, 0, 0, 0);
    b[it] = make_uint4(0, 0, 0, 0);
    if (id < CHUNKS && key < N) {
      a[it] = *reinterpret_cast<const uint4*>(sk + (int64_t)key * ld + c * 8);
      b[it] = *reinterpret_cast<const uint4*>(sv + (int64_t)key * ld + c * 8);
    }
  }
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int id = tid + it * NTHREADS;
    const int key = id >> 3, c = id & 7;
    if (id < CHUNKS) {
      *reinterpret_cast<uint4*>(dk + key * 144 + c * 16) = a[it];
      *reinterpret_cast<uint4*>(dv + key * 144 + c * 16) = b[it];
    }
  }
}
template <int NT, int NTHREADS>
__device__ __forceinline__ void stage_rows_f32(float* dst, const float* src, int64_t ld, int N, int tid) {
  constexpr int CHUNKS = NT * 32 * 16;
  constexpr int ITERS = (CHUNKS + NTHREADS - 1) / NTHREADS;
  constexpr int BATCH = 7;
#pragma unroll 1
  for (int it0 = 0; it0 < ITERS; it0 += BATCH) {
    float4 v[BATCH];
#pragma unroll
    for (int u = 0; u < BATCH; ++u) {
      const int id = tid + (it0 + u) * NTHREADS;
      const int key = id >> 4, c = id & 15;
      v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (id < CHUNKS && key < N) v[u] = *reinterpret_cast<const float4*>(src + (int64_t)key * ld + c * 4);
    }
#pragma unroll
    for (int u = 0; u < BATCH; ++u) {
      const int id = tid + (it0 + u) * NTHREADS;
      const int key = id >> 4, c = id & 15;
      if (id < CHUNKS) {
        float* d = dst + key * 65 + c * 4;
        d[0] = v[u].x; d[1] = v[u].y; d[2] = v[u].z; d[3] = v[u].w;
      }
    }
  }
}

// ---- per-lane operand fragments of one 32-row tile loaded straight from global ----------
template <typename T> struct RowFrag {        // 16-bit storage
  bf16x8_t f[4];
  __device__ __forceinline__ void load(const T* rowp, int half) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) f[ks] = *reinterpret_cast<const bf16x8_t*>(rowp + ks * 16 + half * 8);
  }
};
template <> struct RowFrag<float> {
  float f[32];  // element half*32 + ks
  __device__ __forceinline__ void load(const float* rowp, int half) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float4 v = *reinterpret_cast<const float4*>(rowp + half * 32 + 4 * i);
      f[4 * i] = v.x; f[4 * i + 1] = v.y; f[4 * i + 2] = v.z; f[4 * i + 3] = v.w;
    }
  }
};

// one 32x32 tile:  D[i][q] = M[32t + i][:] . frag[q][:]   (M = K or V rows, row-major in LDS)
template <typename T>
__device__ __forceinline__ f32x16_t tile_times_frag(const char* lds, int t, const RowFrag<T>& fr, int l31, int half) {
  f32x16_t acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  if constexpr (sizeof(T) == 2) {
    const char* rowp = lds + (32 * t + l31) * 144 + half * 16;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const bf16x8_t a = *reinterpret_cast<const bf16x8_t*>(rowp + ks * 32);
      acc = mfma16<T>(a, fr.f[ks], acc);
    }
  } else {
    const float* rowp = reinterpret_cast<const float*>(lds) + (32 * t + l31) * 65 + half * 32;
#pragma unroll
    for (int ks = 0; ks < 32; ++ks) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(rowp[ks], fr.f[ks], acc, 0, 0, 0);
  }
  return acc;
}

// Same product with the frag operand given in "C/D order": cd[ks] = pack8 of registers 8*(ks&1) .. +7 of the 32x32 MFMA
// result tile ks>>1 whose ROWS are this contraction's index, i.e. lane (q, half) holds elements
// j = 16*ks + 4*half + {0..3} and 16*ks + 8 + 4*half + {0..3}.  A k-order applied to both operands cancels, so the LDS
// rows are read as the same two 8-byte pieces -- no lane exchange between the MFMA that produced cd and this one.
template <typename T>
__device__ __forceinline__ f32x16_t tile_times_cdfrag(const char* lds, int t, const bf16x8_t (&cd)[4], int l31, int half) {
  typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;
  typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
  f32x16_t acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const char* rowp = lds + (32 * t + l31) * 144 + half * 8;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    const u32x2 lo = *reinterpret_cast<const u32x2*>(rowp + ks * 32), hi = *reinterpret_cast<const u32x2*>(rowp + ks * 32 + 16);
    u32x4 a; a[0] = lo[0]; a[1] = lo[1]; a[2] = hi[0]; a[3] = hi[1];
    acc = mfma16<T>(__builtin_bit_cast(bf16x8_t, a), cd[ks], acc);
  }
  return acc;
}

// keys >= N of tile t -> -inf (only tiles that can hold padding pay for the compare), then the tile's row
// maximum over both lane halves.  A lane holds one query's scores for 16 of the tile's 32 keys.
__device__ __forceinline__ float mask_and_max(f32x16_t& s, int t, int N, int half) {
  if (32 * t + 32 > N) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * half;
      s[r] = key < N ? s[r] : -INFINITY;
    }
  }
  float m = s[0];
#pragma unroll
  for (int r = 1; r < 16; ++r) m = fmaxf(m, s[r]);
  return fmaxf(m, __shfl_xor(m, 32, 64));
}

// s <- exp((s - m) * scale) element-wise; returns this lane's partial row sum.
// bf16 path: one fma + raw v_exp_f32 per element (arguments <= 0: no range fix-up needed).
template <typename T>
__device__ __forceinline__ float exp_tile(f32x16_t& s, float m, float scale) {
  float l = 0.f;
  if constexpr (sizeof(T) == 2) {
    const float c = scale * LOG2E, mc = m * c;
#pragma unroll
    for (int r = 0; r < 16; ++r) { s[r] = __builtin_amdgcn_exp2f(fmaf(s[r], c, -mc)); l += s[r]; }
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) { s[r] = expf((s[r] - m) * scale); l += s[r]; }
  }
  return l;
}
template <typename T> __device__ __forceinline__ float exp_scalar(float d, float scale) {
  if constexpr (sizeof(T) == 2) return __builtin_amdgcn_exp2f(d * scale * LOG2E);
  else return expf(d * scale);
}

// o[dt] += M^T-contraction:  D[d][q] += sum_key M[key][d] * w[q][key], keys of tile t.
// bf16: M^T fragments parked fragment-major in LDS (frag, [NT][2][2][64][16 B]); f32: M row-major (ms, [NPAD][65]).
template <typename T, int NT>
__device__ __forceinline__ void contract_keys(const char* m_lds, int t, const f32x16_t& w, f32x16_t (&o)[2],
                                              int l31, int half) {
  if constexpr (sizeof(T) == 2) {
    float wf[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) wf[r] = w[r];
    const int lane = l31 + 32 * half;
#pragma unroll
    for (int g2 = 0; g2 < 2; ++g2) {
      const bf16x8_t b = pack8<T>(wf + 8 * g2);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        const bf16x8_t a = *reinterpret_cast<const bf16x8_t*>(m_lds + (((t * 2 + dt) * 2 + g2) * 64 + lane) * 16);
        o[dt] = mfma16<T>(a, b, o[dt]);
      }
    }
  } else {
    const float* ms = reinterpret_cast<const float*>(m_lds);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * half;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
        o[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(ms[key * 65 + 32 * dt + l31], w[r], o[dt], 0, 0, 0);
    }
  }
}

// ---- forward, 16-bit storage, round 6: the key loop ---------------------------------------------------------------------
// What a wave does per key tile is one dependent chain (4 score MFMAs on one accumulator -> max -> cross-half exchange ->
// exp -> rescale of the output tile -> 4 P.V MFMAs) and the workgroup's time is staging + NT of them
// (profiles/r06_attn_timeline.txt: 4.3-8.9 k cycles of staging, 9.5-12 k of loop, with ONE or TWO workgroups on the CU alike).
//  * THE PARTIAL KEY TILE (N = 197 = 6 x 32 + 5; 257 = 8 x 32 + 1) is peeled: by the C/D map a lane's registers 4g .. 4g+3
//    are key offsets 8g + 4 half + {0..3}, so with rem valid keys only G = ceil(rem / 8) register groups are live -- the
//    exps, sums and conversions of the others and the P.V MFMAs of a 16-key half without live keys are not issued
//    (rem = 5: 4 of 16 v_exp, 2 of 4 P.V MFMAs); key tiles past N (N < 32 (NT - 1)) are skipped.  What is skipped is
//    arithmetic on exact zeros (exp2(-inf) = 0, 0 x v, alpha = 1), so the result is BIT-IDENTICAL to the round-5 kernel.
// (The build-time arms of rounds 4 to 6 -- lazy rescale, two key tiles per trip, K by LDS-DMA, the two-pass softmaxes, split
//  units -- were measured and not adopted: DESIGN.md 5c and the profiles named there; git history has their code.)

// moves the running maximum m to cover this tile's row maximum tm; returns the factor the running sum / output carry
template <typename T>
__device__ __forceinline__ float move_max(float tm, float scale, float& m, f32x16_t (&o)[2]) {
  const float mn = fmaxf(m, tm);                            // finite from the first tile on (N >= 1)
  const float alpha = exp_scalar<T>(m - mn, scale);         // first tile: exp(-inf) = 0
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
  m = mn;
  return alpha;
}

// the PARTIAL key tile: rem = N - 32 t valid keys, G = ceil(rem / 8) live register groups of four (wave-uniform branches:
// one code path for every G -- four template instances of it spilled 35 registers around a switch)
template <typename T, int NT>
__device__ __forceinline__ void fwd_tile_tail(const char* ks, const char* vs, int t, int rem, const RowFrag<T>& qf,
                                              float scale, float& m, float& l, f32x16_t (&o)[2], int l31, int half) {
  f32x16_t sc = tile_times_frag<T>(ks, t, qf, l31, half);      // (K rows >= N hold zeros: finite scores)
  const int G = (rem + 7) >> 3;
  float tm = -INFINITY;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    if (g < G) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = 4 * g + j, off = j + 8 * g + 4 * half;
        sc[r] = off < rem ? sc[r] : -INFINITY;
        tm = fmaxf(tm, sc[r]);
      }
    }
  }
  tm = fmaxf(tm, __shfl_xor(tm, 32, 64));                      // finite: offset 0 is valid and belongs to half 0
  const float alpha = move_max<T>(tm, scale, m, o);
  const float c = scale * LOG2E, mc = m * c;
  float p[16], lt = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) p[r] = 0.f;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    if (g < G) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {                            // exp2(-inf) = 0 for the masked offsets of the last group
        p[4 * g + j] = __builtin_amdgcn_exp2f(fmaf(sc[4 * g + j], c, -mc));
        lt += p[4 * g + j];
      }
    }
  }
  l = l * alpha + lt;
  const int lane = l31 + 32 * half;
#pragma unroll
  for (int g2 = 0; g2 < 2; ++g2) {
    if (2 * g2 < G) {
      const bf16x8_t b = pack8<T>(p + 8 * g2);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        const bf16x8_t a = *reinterpret_cast<const bf16x8_t*>(vs + (((t * 2 + dt) * 2 + g2) * 64 + lane) * 16);
        o[dt] = mfma16<T>(a, b, o[dt]);
      }
    }
  }
}

// ---- forward: the pieces every forward kernel is made of ---------------------------------------------------------------
// Online softmax of one query tile over the staged key tiles [ta, tb): running maximum m, running sum l, output tile o
// rescaled when m grows -- only one score tile is live, so the kernels fit 128 VGPRs and TWO workgroups share a CU.
// m, l and o carry over from call to call (the two-phase kernel's phases, the long kernel's chunks).
//   16-bit: full tiles (no key to mask), then, if rem > 0, the partial tile tb with its rem keys (fwd_tile_tail);
//   f32   : every tile masked against N (rem unused).
// l31 must be an opaque copy made inside the caller's query-tile loop: K / V in LDS do not depend on the query tile, and
// without the copy the compiler hoists all of their ds_reads out of that loop and spills them to scratch.
template <typename T, int NT>
__device__ __forceinline__ void fwd_walk_keys(const char* ks, const char* vs, int ta, int tb, int rem, int N,
                                              const RowFrag<T>& qf, float scale, float& m, float& l, f32x16_t (&o)[2],
                                              int l31, int half) {
  if constexpr (sizeof(T) == 2) {
#pragma unroll 1
    for (int t = ta; t < tb; ++t) {
      f32x16_t sc = tile_times_frag<T>(ks, t, qf, l31, half);
      float tm = sc[0];
#pragma unroll
      for (int r = 1; r < 16; ++r) tm = fmaxf(tm, sc[r]);
      tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
      const float alpha = move_max<T>(tm, scale, m, o);
      l = l * alpha + exp_tile<T>(sc, m, scale);
      contract_keys<T, NT>(vs, t, sc, o, l31, half);
    }
    if (rem > 0) fwd_tile_tail<T, NT>(ks, vs, tb, rem, qf, scale, m, l, o, l31, half);
  } else {
#pragma unroll 1
    for (int t = ta; t < tb; ++t) {
      // (issuing the score tile of key tile t+1 before the softmax arithmetic of tile t -- one more live tile, 118 VGPRs --
      //  measured nothing: loop 9.5 k vs 9.7 k cycles per workgroup, in-step 14.7 vs 13.6 us, step 3.008 vs 3.009 ms)
      f32x16_t sc = tile_times_frag<T>(ks, t, qf, l31, half);
      const float mn = fmaxf(m, mask_and_max(sc, t, N, half));     // finite from the first tile that holds a key on
      const float alpha = exp_scalar<T>(m - mn, scale);           // first tile: exp(-inf) = 0
      l = l * alpha + exp_tile<T>(sc, mn, scale);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
      contract_keys<T, NT>(vs, t, sc, o, l31, half);
      m = mn;
    }
  }
}
__device__ __forceinline__ void fwd_reset(float& m, float& l, f32x16_t (&o)[2]) {
  m = -INFINITY; l = 0.f;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
}

// row <- mul * tile: lane (l31, half) holds elements 32 dt + 8 g + 4 half + {0..3} of its query's row
template <typename T>
__device__ __forceinline__ void store_tile(T* orow, const f32x16_t (&o)[2], float mul, int half) {
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      ActIO<T>::st4(orow + 32 * dt + 8 * g + 4 * half, o[dt][4 * g] * mul, o[dt][4 * g + 1] * mul, o[dt][4 * g + 2] * mul,
                    o[dt][4 * g + 3] * mul);
}
// the end of a query tile: the row sum over both lane halves, out row = o / l if this lane's query is wanted
template <typename T>
__device__ __forceinline__ void fwd_store_tile(T* orow, const f32x16_t (&o)[2], float l, bool wanted, int half) {
  l += __shfl_xor(l, 32, 64);
  const float inv = 1.0f / l;
  if (wanted) store_tile<T>(orow, o, inv, half);
}

// V^T fragments of key tile t from its 32 rows (vrows: row l31's four 16-B pieces of this lane's half): transposed on the
// matrix core and parked fragment-major, [NT][2 dt][2 g2][64 lanes][16 B], where contract_keys / fwd_tile_tail read them
template <typename T>
__device__ __forceinline__ void stage_vt(char* vs, int t, const bf16x8_t (&vrows)[4], const bf16x8_t& i0,
                                         const bf16x8_t& i1, int lane) {
#pragma unroll
  for (int dt = 0; dt < 2; ++dt) {
    bf16x8_t fr[2];
    transpose_tile<T>(vrows, dt, i0, i1, fr);
#pragma unroll
    for (int g2 = 0; g2 < 2; ++g2)
      *reinterpret_cast<bf16x8_t*>(vs + (((t * 2 + dt) * 2 + g2) * 64 + lane) * 16) = fr[g2];
  }
}
// The V rows of the key tiles wave w transposes (w, w + 8), with ordinary loads: load() only issues them -- the caller puts
// its other requests behind them -- and park() stages their V^T fragments.  Rows at or past N are zeros.
template <typename T, int NT> struct VtRows {
  static constexpr int NVT = (NT + 7) / 8;
  bf16x8_t rows[NVT][4];
  __device__ __forceinline__ void load(const T* vb, int64_t ld, int N, int wave, int l31, int half) {
#pragma unroll
    for (int ti = 0; ti < NVT; ++ti) {
      const int key = 32 * (wave + 8 * ti) + l31;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        uint4 z = make_uint4(0, 0, 0, 0);
        if ((NT % 8 == 0 || wave + 8 * ti < NT) && key < N)
          z = *reinterpret_cast<const uint4*>(vb + (int64_t)key * ld + kk * 16 + half * 8);
        rows[ti][kk] = __builtin_bit_cast(bf16x8_t, z);
      }
    }
  }
  __device__ __forceinline__ void park(char* vs, int wave, int lane, int l31, int half) const {
    const bf16x8_t i0 = ident_frag<T>(0, l31, half), i1 = ident_frag<T>(1, l31, half);
#pragma unroll
    for (int ti = 0; ti < NVT; ++ti) {
      const int t = wave + 8 * ti;
      if (NT % 8 == 0 || t < NT) stage_vt<T>(vs, t, rows[ti], i0, i1, lane);
    }
  }
};

// Workgroup i of n -> its (image, head) unit.  Block i runs on XCD i % 8: every XCD takes a contiguous run of (image, head)
// pairs, i.e. whole images -- the images whose rows the out-proj / c_fc / c_proj kernels around this one handle on the same
// XCD (row units).
__device__ __forceinline__ int xcd_unit(int i, int n) {
  const int qd = n >> 3, rm = n & 7, xcd = i & 7;
  return (xcd < rm ? xcd * (qd + 1) : rm * (qd + 1) + (xcd - rm) * qd) + (i >> 3);
}
// query s (clamped to the last one, S - 1 = N + Kp - 1) of image b in the engine's row layout: B N frozen rows | B Kp prompt rows
__device__ __forceinline__ int64_t frozen_prompt_row(int s, int b, int B, int N, int Kp, int S) {
  const int sc = min(s, S - 1);
  return sc < N ? (int64_t)b * N + sc : (int64_t)B * N + (int64_t)b * Kp + (sc - N);
}
// query vq (clamped to the last one, Q - 1 = sets Kp - 1) of image b in the set-major prompt rows: row (s B + b) Kp + j
__device__ __forceinline__ int64_t set_major_row(int vq_, int b, int B, int Kp, int Q) {
  const int vq = min(vq_, Q - 1);
  const int s = vq / Kp, j = vq - s * Kp;
  return ((int64_t)s * B + b) * Kp + j;
}

// ---- forward ---------------------------------------------------------------------------
template <typename T, int NT>
__global__ __launch_bounds__(512, 4) void attn_fwd_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                       const T* __restrict__ v, int64_t ld, T* out,
                                                       int64_t ldo, int B, int H, int N, int Kp, float scale,
                                                       int q_first) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using L = AL<T, NT>;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, l31 = lane & 31;
  const int unit = xcd_unit(blockIdx.x, gridDim.x);
  const int b = unit / H, h = unit % H;
  const T* kb = k + (int64_t)b * N * ld + h * 64;
  const T* vb = v + (int64_t)b * N * ld + h * 64;
  char* ks = smem;
  char* vs = smem + L::K_BYTES;
  const int S = N + Kp;
  RPO_STAMP(0);
  // every HBM round trip of the prologue is issued up front: this wave's first query fragment, its V rows
  // (bf16: the key tile it transposes), then the K staging loads
  auto qrow = [&](int qt) { return frozen_prompt_row(qt * 32 + l31, b, B, N, Kp, S); };
  RowFrag<T> qf;
  // q_first > 0: only queries q_first .. S-1 of every image are wanted (last block: the prompt rows); whole
  // 32-query tiles are skipped, the leading queries of the first computed tile are computed but not stored
  const int qt0 = q_first >> 5, qt_end = (S + 31) >> 5;
  if constexpr (sizeof(T) == 2) qf.load(q + qrow(qt0 + wave) * ld + h * 64, half);   // (f32: 32 live VGPRs too many)
  if constexpr (sizeof(T) == 2) {
    VtRows<T, NT> vt;
    vt.load(vb, ld, N, wave, l31, half);
    stage_rows_bf16<NT, 512>(ks, reinterpret_cast<const bf16_t*>(kb), ld, N, tid);
    RPO_STAMP(1);
    vt.park(vs, wave, lane, l31, half);
  } else {
    stage_rows_f32<NT, 512>(reinterpret_cast<float*>(ks), kb, ld, N, tid);
    stage_rows_f32<NT, 512>(reinterpret_cast<float*>(vs), vb, ld, N, tid);
  }
  RPO_STAMP(2);
  __syncthreads();
  RPO_STAMP(3);
  // 16-bit: the full key tiles, the partial one peeled, key tiles past N skipped (see fwd_tile_tail); f32: all NT tiles, masked
  const int nfull = sizeof(T) == 2 ? min(N >> 5, NT) : NT, rem = nfull < NT ? N - 32 * nfull : 0;
  for (int qt = qt0 + wave; qt < qt_end; qt += 8) {
    int l31v = l31;                                      // (opaque copy: see fwd_walk_keys)
    asm volatile("" : "+v"(l31v));
    const int s = qt * 32 + l31;
    const int64_t grow = qrow(qt);
    if (sizeof(T) != 2 || qt != qt0 + wave) qf.load(q + grow * ld + h * 64, half);
    float m, l;
    f32x16_t o[2];
    fwd_reset(m, l, o);
    fwd_walk_keys<T, NT>(ks, vs, 0, nfull, rem, N, qf, scale, m, l, o, l31v, half);
    fwd_store_tile<T>(out + grow * ldo + h * 64, o, l, s < S && s >= q_first, half);
    RPO_STAMP(6);
  }
#ifdef RPO_TIMELINE
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
  RPO_STAMP(7);
}

// ---- forward, 16-bit storage, round 6: the key loop STARTS while the tail of K is still in flight ------------------------
// profiles/r06_attn_timeline.txt: of a workgroup's 16.6 k (one per CU) .. 25 k (two per CU) cycles, 4.3 .. 8.9 k pass before
// the staging barrier -- all 384 workgroups of a launch pull their 57 KB of K / V at once, ~41 MB at the rate the fabric
// delivers -- and the key loop (7 dependent chains of ~1.4 k cycles) cannot start before the LAST byte has landed.  Here:
//  * every request of the prologue is issued up front in the order q fragment, V rows, K rows [0, 128) (phase A), the rest
//    of K (phase B) -- K as 16-B register loads into the 144-B padded rows of attn_fwd_kernel;
//  * the waves retire them with COUNTED waits: q + V -> V^T fragments on the matrix core; phase A -> barrier A -> the key
//    loop over key tiles 0 .. 3; phase B -> barrier B -> the remaining tiles.  Left to hipcc the V loads sink into the
//    `tile < NT` branch that uses them and every wait merges to vmcnt(0) (ISA of the first version) -- hence inline asm
//    for the issue and the waits; the compiler issues no vector-memory instruction of its own before barrier B.
//  * its VGPR budget (110 at NT = 7) decides whether the side queue's waves fit beside two workgroups per CU
//    (same-box step time by VGPR budget of this kernel: profiles/r06_attn_variants.txt).
// Arithmetic per query row is that of attn_fwd_kernel: bit-identical results.
template <typename T, int NT> struct AL16 {
  static constexpr int NPAD = NT * 32;
  static constexpr int K_BYTES = NPAD * 144;                     // rows padded to 144 B
  static constexpr int F_BYTES = NT * 4 * 1024;                  // V^T fragments
  static constexpr int BYTES = K_BYTES + F_BYTES;
  static constexpr int NKR = (NPAD / 8 + 7) / 8;                 // K requests per thread (= ceil(NPAD * 8 / 512))
};

template <typename T, int NT>
__global__ __launch_bounds__(512, 4) void attn_fwd16_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                         const T* __restrict__ v, int64_t ld, T* out,
                                                         int64_t ldo, int B, int H, int N, int Kp, float scale,
                                                         int q_first) {
  static_assert(sizeof(T) == 2, "16-bit storage only");
  extern __shared__ __attribute__((aligned(128))) char smem[];
  using L = AL16<T, NT>;
  // K requests per thread: 16-B register loads (thread t: chunk t + 512 i); phase A = the first PH of them = K rows [0, 128)
  constexpr int NKR = L::NKR, PH = 2;
  static_assert(NKR > PH && NKR <= 5, "the counted waits below are written out for 3 .. 5 requests");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5, l31 = lane & 31;
  const int unit = xcd_unit(blockIdx.x, gridDim.x);
  const int b = unit / H, h = unit % H;
  const T* kb = k + (int64_t)b * N * ld + h * 64;
  const T* vb = v + (int64_t)b * N * ld + h * 64;
  char* ks = smem;
  char* vs = smem + L::K_BYTES;
  const int S = N + Kp;
  RPO_STAMP(0);
  auto qrow = [&](int qt) { return frozen_prompt_row(qt * 32 + l31, b, B, N, Kp, S); };
  const int qt0 = q_first >> 5, qt_end = (S + 31) >> 5;
  const int qt_mine = qt0 + wave;
  typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
  constexpr int NVT = (NT + 7) / 8;
  RowFrag<T> qf;
  u32x4 qreg[4], vreg[NVT][4], kreg[NKR];
  {
    const T* qp = q + qrow(qt_mine) * ld + h * 64 + half * 8;      // (rows are clamped: waves without a tile load a valid row)
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
      asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(qreg[kk]) : "v"(qp + kk * 16) : "memory");
#pragma unroll
    for (int ti = 0; ti < NVT; ++ti) {
      const T* vp = vb + (int64_t)min(32 * (wave + 8 * ti) + l31, N - 1) * ld + half * 8;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
        asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(vreg[ti][kk]) : "v"(vp + kk * 16) : "memory");
    }
    // K: rows >= N re-read row N - 1 (commit_k zeroes them); a chunk past the panel is loaded and not written
#pragma unroll
    for (int i = 0; i < NKR; ++i) {
      const int id = tid + i * 512;
      const T* kp = kb + (int64_t)min(id >> 3, N - 1) * ld + (id & 7) * 8;
      asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(kreg[i]) : "v"(kp) : "memory");
    }
  }
  // chunk id = tid + 512 i of the [NPAD][8]-chunk K panel -> its padded LDS row; rows >= N are zeroed
  auto commit_k = [&](int i) {
    const int id = tid + i * 512;
    const int key = id >> 3, c = id & 7;
    const u32x4 z = {0u, 0u, 0u, 0u};
    if (id < L::NPAD * 8) *reinterpret_cast<u32x4*>(ks + key * 144 + c * 16) = key < N ? kreg[i] : z;
  };
  // q and V have landed once at most the NKR K requests are outstanding (returns are in order)
  if constexpr (NVT == 1)
    asm volatile("s_waitcnt vmcnt(%8)" : "+v"(qreg[0]), "+v"(qreg[1]), "+v"(qreg[2]), "+v"(qreg[3]), "+v"(vreg[0][0]),
                 "+v"(vreg[0][1]), "+v"(vreg[0][2]), "+v"(vreg[0][3]) : "n"(NKR) : "memory");
  else
    asm volatile("s_waitcnt vmcnt(%12)" : "+v"(qreg[0]), "+v"(qreg[1]), "+v"(qreg[2]), "+v"(qreg[3]), "+v"(vreg[0][0]),
                 "+v"(vreg[0][1]), "+v"(vreg[0][2]), "+v"(vreg[0][3]), "+v"(vreg[NVT - 1][0]), "+v"(vreg[NVT - 1][1]),
                 "+v"(vreg[NVT - 1][2]), "+v"(vreg[NVT - 1][3]) : "n"(NKR) : "memory");
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) qf.f[kk] = __builtin_bit_cast(bf16x8_t, qreg[kk]);
  // V^T fragments: wave w transposes key tiles w, w + 8 on the matrix core (rows >= N contribute zeros)
  {
    const bf16x8_t i0 = ident_frag<T>(0, l31, half), i1 = ident_frag<T>(1, l31, half);
    const u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int ti = 0; ti < NVT; ++ti) {
      const int t = wave + 8 * ti;
      if (t < NT) {
        bf16x8_t vrows[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) vrows[kk] = __builtin_bit_cast(bf16x8_t, 32 * t + l31 < N ? vreg[ti][kk] : z);
        stage_vt<T>(vs, t, vrows, i0, i1, lane);
      }
    }
  }
  RPO_STAMP(1);
  asm volatile("s_waitcnt vmcnt(%1)" : "+v"(kreg[0]) : "n"(NKR - 1) : "memory");
  commit_k(0);
  asm volatile("s_waitcnt vmcnt(%1)" : "+v"(kreg[1]) : "n"(NKR - 2) : "memory");
  commit_k(1);
  RPO_STAMP(2);
  __syncthreads();                                               // barrier A: V^T of every tile, K rows [0, 128)
  RPO_STAMP(3);
  const int nfull = min(N >> 5, NT), rem = nfull < NT ? N - 32 * nfull : 0;   // full key tiles; keys of the partial one
  const int nA = min(nfull, 2 * PH);                             // full key tiles inside phase A's rows
  float m, l;
  f32x16_t o[2];
  fwd_reset(m, l, o);
  auto store = [&](int qt) {
    const int s = qt * 32 + l31;
    fwd_store_tile<T>(out + qrow(qt) * ldo + h * 64, o, l, s < S && s >= q_first, half);
  };
  int l31v = l31;                                                // (opaque copy: see fwd_walk_keys)
  asm volatile("" : "+v"(l31v));
  const bool have = qt_mine < qt_end;                            // (wave-uniform)
  if (have) fwd_walk_keys<T, NT>(ks, vs, 0, nA, 0, N, qf, scale, m, l, o, l31v, half);
  RPO_STAMP(4);
  asm volatile("s_waitcnt vmcnt(%1)" : "+v"(kreg[2]) : "n"(NKR - 3) : "memory");
  commit_k(2);
  if constexpr (NKR > 3) {
    asm volatile("s_waitcnt vmcnt(%1)" : "+v"(kreg[NKR > 3 ? 3 : 0]) : "n"(NKR > 3 ? NKR - 4 : 0) : "memory");
    commit_k(3);
  }
  if constexpr (NKR > 4) {
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(kreg[NKR - 1]) : : "memory");
    commit_k(NKR - 1);
  }
  __syncthreads();                                               // barrier B: the rest of K
  RPO_STAMP(5);
  if (have) {
    fwd_walk_keys<T, NT>(ks, vs, nA, nfull, rem, N, qf, scale, m, l, o, l31v, half);
    store(qt_mine);
  }
  RPO_STAMP(6);
  for (int qt = qt_mine + 8; qt < qt_end; qt += 8) {             // (S > 256: ViT-L/14's ninth query tile)
    asm volatile("" : "+v"(l31v));
    qf.load(q + qrow(qt) * ld + h * 64, half);
    fwd_reset(m, l, o);
    fwd_walk_keys<T, NT>(ks, vs, 0, nfull, rem, N, qf, scale, m, l, o, l31v, half);
    store(qt);
  }
#ifdef RPO_TIMELINE
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
  RPO_STAMP(7);
}

// ---- backward (prompt rows only; dq) -----------------------------------------------------
// dq = scale * (U - delta * W),  U = sum_key (p*dp)[key] K[key],  W = sum_key p[key] K[key],
// delta = sum_key p*dp, dp = da . V^T.  One pass over the key tiles, no saved forward output.
// The 4 waves of the workgroup share one 32-query tile: each recomputes the (cheap) score tile row
// statistics, then takes the key tiles t = wave, wave+4, ... for dP / U / W; partial U, W, delta are
// combined through LDS (the staging area is dead by then).
//
// bwd_pass2_tile is the pass-2 step of one key tile, written once for attn_bwd_body (all keys staged at once) and
// attn_bwd_long_kernel (the keys in chunks), both storage forms and both forms of `da`.  The pass-1 tile step, the rowstat
// merge, the partial combine with the dq store and the dS . K contraction of attn_prompt_bwd_kernel are stated per kernel on
// purpose: as helpers they change the register allocation (profiles/image_attn_bwd_refactor_ab.txt).
//
// Pass 2, one key tile: P from the merged (m, 1 / l), dP = da . V^T, delta += sum P o dP, and the contractions
// u (U) += (P o dP) . K, w (W) += P . K.  `da` is this lane's query row of d(attention output): a RowFrag, or
// -- folded d out-proj -- the four fragments in C/D order that the prologue of attn_bwd_body leaves (tile_times_cdfrag).
template <typename T, int NT, typename DA>
__device__ __forceinline__ void bwd_pass2_tile(const char* ks, const char* vs, int t, int N, const RowFrag<T>& qf,
                                               const DA& da, float m, float inv, float scale, f32x16_t (&u)[2], f32x16_t (&w)[2],
                                               float& delta, const bf16x8_t& i0, const bf16x8_t& i1, int l31, int half) {
  f32x16_t pt = tile_times_frag<T>(ks, t, qf, l31, half);
  (void)mask_and_max(pt, t, N, half);
  (void)exp_tile<T>(pt, m, scale);
  f32x16_t dp;
  if constexpr (std::is_same<DA, RowFrag<T>>::value) dp = tile_times_frag<T>(vs, t, da, l31, half);
  else dp = tile_times_cdfrag<T>(vs, t, da, l31, half);
  if constexpr (sizeof(T) == 2) {
    const char* krow = ks + (32 * t + l31) * 144 + half * 16;
    bf16x8_t krows[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) krows[kk] = *reinterpret_cast<const bf16x8_t*>(krow + kk * 32);
    float pw[16], pp[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      pp[r] = pt[r] * inv;
      pw[r] = dp[r] * pp[r];                       // P * dP  (P = 0 on padded keys)
      delta += pw[r];
    }
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      bf16x8_t ktf[2];
      transpose_tile<T>(krows, dt, i0, i1, ktf);   // K^T fragments of this key tile, in registers
#pragma unroll
      for (int g2 = 0; g2 < 2; ++g2) {
        u[dt] = mfma16<T>(ktf[g2], pack8<T>(pw + 8 * g2), u[dt]);
        w[dt] = mfma16<T>(ktf[g2], pack8<T>(pp + 8 * g2), w[dt]);
      }
    }
  } else {
    f32x16_t pn;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      pn[r] = pt[r] * inv;
      dp[r] *= pn[r];
      delta += dp[r];
    }
    contract_keys<T, NT>(ks, t, dp, u, l31, half);
    contract_keys<T, NT>(ks, t, pn, w, l31, half);
  }
}

// NCW > 0 (16-bit storage): the d out-proj GEMM is folded in.  `da` then is d(out-proj output) [B*Kp, d] (d = 256 * NCW)
// and `wo` the transposed out-proj weight [d (in), d (out)]: the workgroup first forms its head's slice
// da_h = da . W_out[:, 64h .. 64h+63] -- 32 x 64 x d on the matrix cores, the four waves taking d / 4 of the contraction
// each, operands straight from global memory in one batch with the K / V staging loads, partial tiles summed through LDS
// before K / V land there -- and feeds it to the dP MFMAs in the layout the result tile already has
// (tile_times_cdfrag).  One launch and one [B*Kp, d] round trip per block less on the backward chain.
template <typename T, int NT, int NCW>
// (No __restrict__ on the inputs: hipcc treats loads through restrict-const pointers as invariant and moves them across
// the asm memory barriers that pin the order of the fused prologue's loads -- its vmcnt waits are counted.)
// (bid, nwg): this problem's workgroup index / count (the whole grid in a plain launch, its share of the grid in a paired
// one).  key_len / key_stride: group b reads keys [0, key_len[b]) of the key_stride rows that k / v hold per group (the text
// tower's per-class K / V cache: trainers/rpo.py:144-151 -- a prompt row of class c reads exactly the len_c frozen tokens);
// key_len == nullptr: every group has N keys stored back to back (the image tower).
__device__ __forceinline__ void attn_bwd_body(char* smem, const int bid, const int nwg,
                                              const T* qr, int64_t ldq, const T* k, const T* v,
                                              int64_t ldkv, const T* da, int64_t ldda,
                                              T* dq, int64_t lddq, int B, int H, int N, int Kp,
                                              float scale, const T* wo, int64_t ldwo,
                                              const int32_t* key_len, int key_stride, const bool plain_order = false,
                                              const int nqt_wg = 1) {
  using L = AL<T, NT>;
  // fused variant: every wave owns WSLOTS 8-KiB landing slots for its W_out^T chunks (NCW <= 3: two, the third chunk re-uses
  // slot 0; NCW = 4, d = 1024: four, all requested up front)
  constexpr int WSLOTS = NCW == 4 ? 4 : 2, WSTRIDE = WSLOTS * 8192;
  constexpr int stat_off = NCW > 0 && L::BWD_BYTES < 4 * WSTRIDE ? 4 * WSTRIDE : L::BWD_BYTES;   // launchers allocate stat_off + 2048
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5, l31 = lane & 31;
  // (plain_order: bid IS the (group, head) index -- the persistent chain kernel, chain.hip, places its items itself)
  const int wgid = plain_order ? bid : xcd_unit(bid, nwg);
  // fused variant with Kp > 32: nqt_wg workgroups per (group, head), one per 32-query tile (adjacent: same XCD)
  const int pair_id = wgid / nqt_wg, qt_wg = wgid - pair_id * nqt_wg;
  const int b = pair_id / H, h = pair_id % H;
  if (key_len != nullptr) N = max(1, min(key_len[b], min(key_stride, NT * 32)));   // keys of this group
  else key_stride = N;
  const T* kb = k + (int64_t)b * key_stride * ldkv + h * 64;
  const T* vb = v + (int64_t)b * key_stride * ldkv + h * 64;
  char* ks = smem;
  char* vs = smem + L::K_BYTES;
  float4* part_u = reinterpret_cast<float4*>(smem);                 // [4 waves][8 groups][64 lanes]
  float4* part_w = part_u + 4 * 8 * 64;
  float* part_d = reinterpret_cast<float*>(part_w + 4 * 8 * 64);    // [4 waves][64 lanes]
  bf16x8_t i0, i1;
  if constexpr (sizeof(T) == 2) { i0 = ident_frag<T>(0, l31, half); i1 = ident_frag<T>(1, l31, half); }

  // fused variant: one query tile (the launcher checks Kp <= 32) -- with a runtime trip count hipcc hoists the address
  // arithmetic of every load of the prologue out of the loop and spills it
  const int nqt = NCW > 0 ? 1 : (Kp + 31) / 32;
  for (int qt0 = 0; qt0 < nqt; ++qt0) {
    if (qt0 > 0) __syncthreads();                  // partials of the previous tile have been consumed
    const int qt = NCW > 0 ? qt_wg : qt0;
    const int i = qt * 32 + l31;
    const int64_t prow = (int64_t)b * Kp + min(i, Kp - 1);
    RowFrag<T> qf, df;                             // issued ahead of the staging loads: one HBM round trip
    RPO_STAMP(10);
    qf.load(qr + prow * ldq + h * 64, half);
    bf16x8_t dcd[4];                               // fused path: da_h of this lane's query in C/D order
    if constexpr (NCW > 0) {
      static_assert(sizeof(T) == 2, "the fused d out-proj needs 16-bit storage");
      // This wave's NCW 64-deep chunks of the contraction (chunks wave, wave + 4, ...).  The W_out^T slice (64 rows x 128 B
      // per chunk) comes in by LDS-DMA into two wave-private 8-KB slots -- whole 128-B lines per 8 lanes, XOR-swizzled
      // like the GEMM tiles; as per-lane operand loads (32 rows x 32 B per instruction) the same bytes took 16 k cycles --
      // the dx rows as per-lane fragments, and K / V are requested behind them so that their (cold) latency hides under
      // the MFMAs.  The order of the groups is pinned (counted vmcnt waits below).
      typedef const __attribute__((address_space(1))) void* gptr_t;
      typedef __attribute__((address_space(3))) void* lptr_t;
      char* myslot = smem + wave * WSTRIDE;
      const int dr = lane >> 3, dc = lane & 7;
      const char* wsrc = reinterpret_cast<const char*>(wo) + ((int64_t)(h * 64 + dr) * ldwo) * 2 + 128 * wave;
      auto dma_chunk = [&](int c, int slot) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int sw = ((8 * i + dr) >> 1) & 7;
          __builtin_amdgcn_global_load_lds((gptr_t)(wsrc + (int64_t)(8 * i) * ldwo * 2 + 512 * c + ((dc ^ sw) << 4)),
                                           (lptr_t)(myslot + slot * 8192 + i * 1024), 16, 0, 0);
        }
      };
      dma_chunk(0, 0);
      asm volatile("" ::: "memory");
      dma_chunk(1, 1);
      asm volatile("" ::: "memory");
      if constexpr (NCW == 4) {
        dma_chunk(2, 2);
        asm volatile("" ::: "memory");
        dma_chunk(3, 3);
        asm volatile("" ::: "memory");
      }
      bf16x8_t xb[NCW][4];
      const T* xrow = da + prow * ldda + half * 8 + 64 * wave;
#pragma unroll
      for (int c = 0; c < NCW; ++c)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) xb[c][kk] = *reinterpret_cast<const bf16x8_t*>(xrow + (256 * c + 16 * kk));
      asm volatile("" ::: "memory");
      constexpr int CHUNKS = NT * 32 * 8, ITERS = (CHUNKS + 255) / 256;
      constexpr int NXQ = 4 * NCW;                 // the xb loads (qf was requested before the first DMA: older)
      f32x16_t dpart[2];
#pragma unroll
      for (int jt = 0; jt < 2; ++jt)
#pragma unroll
        for (int r = 0; r < 16; ++r) dpart[jt][r] = 0.f;
      const int fsw = (l31 >> 1) & 7;
      auto mfma_chunk = [&](int c, int slot) {
        const char* base = myslot + slot * 8192 + l31 * 128;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const int off = ((2 * kk + half) ^ fsw) << 4;
          const bf16x8_t a0 = *reinterpret_cast<const bf16x8_t*>(base + off);
          const bf16x8_t a1 = *reinterpret_cast<const bf16x8_t*>(base + 32 * 128 + off);
          dpart[0] = mfma16<T>(a0, xb[c][kk], dpart[0]);
          dpart[1] = mfma16<T>(a1, xb[c][kk], dpart[1]);
        }
      };
      // younger than chunk 0: chunk 1 (8) + xb / qf
      asm volatile("s_waitcnt vmcnt(%0)" :: "n"((NCW == 4 ? 24 : 8) + NXQ) : "memory");
      mfma_chunk(0, 0);
      if constexpr (NCW == 3) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");         // slot 0 has been read
        dma_chunk(2, 0);
        asm volatile("" ::: "memory");
      }
      uint4 ka[ITERS], va[ITERS];
#pragma unroll
      for (int it = 0; it < ITERS; ++it) {         // unconditional (clamped) loads: a branch per load serialises them
        const int id = tid + it * 256, key = min(id >> 3, N - 1), c = id & 7;
        ka[it] = *reinterpret_cast<const uint4*>(kb + (int64_t)key * ldkv + c * 8);
        va[it] = *reinterpret_cast<const uint4*>(vb + (int64_t)key * ldkv + c * 8);
      }
      asm volatile("s_waitcnt vmcnt(%0)" :: "n"(NXQ + (NCW == 3 ? 8 : NCW == 4 ? 16 : 0) + 2 * ITERS) : "memory");   // younger than chunk 1
      mfma_chunk(1, 1);
      if constexpr (NCW == 4) {
        asm volatile("s_waitcnt vmcnt(%0)" :: "n"(NXQ + 8 + 2 * ITERS) : "memory");                    // younger than chunk 2
        mfma_chunk(2, 2);
        asm volatile("s_waitcnt vmcnt(%0)" :: "n"(NXQ + 2 * ITERS) : "memory");                        // younger than chunk 3
        mfma_chunk(3, 3);
      }
      if constexpr (NCW == 3) {
        asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * ITERS) : "memory");                            // younger than chunk 2
        mfma_chunk(2, 0);
      }
      RPO_STAMP(11);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      float4* px = reinterpret_cast<float4*>(myslot);              // this wave's partial tiles: [8][64 lanes], in its own slot
#pragma unroll
      for (int i = 0; i < 8; ++i)
        px[i * 64 + lane] = make_float4(dpart[i >> 2][4 * (i & 3)], dpart[i >> 2][4 * (i & 3) + 1],
                                        dpart[i >> 2][4 * (i & 3) + 2], dpart[i >> 2][4 * (i & 3) + 3]);
      __syncthreads();
      float dfull[32];
      const float4* pall = reinterpret_cast<const float4*>(smem);   // wave w's partials start at byte WSTRIDE * w
      constexpr int PW = WSTRIDE / 16;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float4 a = pall[i * 64 + lane], b = pall[PW + i * 64 + lane], c = pall[2 * PW + i * 64 + lane],
                     d = pall[3 * PW + i * 64 + lane];
        dfull[4 * i] = (a.x + b.x) + (c.x + d.x); dfull[4 * i + 1] = (a.y + b.y) + (c.y + d.y);
        dfull[4 * i + 2] = (a.z + b.z) + (c.z + d.z); dfull[4 * i + 3] = (a.w + b.w) + (c.w + d.w);
      }
#pragma unroll
      for (int ks2 = 0; ks2 < 4; ++ks2) dcd[ks2] = pack8<T>(dfull + 8 * ks2);
      __syncthreads();                             // the partials have been read: K / V may land on them
      RPO_STAMP(12);
#pragma unroll
      for (int it = 0; it < ITERS; ++it) {
        const int id = tid + it * 256, key = id >> 3, c = id & 7;
        if (id < CHUNKS) {
          const bool live = key < N;               // rows past the last key: zeros
          *reinterpret_cast<uint4*>(ks + key * 144 + c * 16) = live ? ka[it] : make_uint4(0, 0, 0, 0);
          *reinterpret_cast<uint4*>(vs + key * 144 + c * 16) = live ? va[it] : make_uint4(0, 0, 0, 0);
        }
      }
    } else if constexpr (sizeof(T) == 2) {
      df.load(da + prow * ldda + h * 64, half);
      stage2_bf16<NT, 256>(ks, vs, reinterpret_cast<const bf16_t*>(kb), reinterpret_cast<const bf16_t*>(vb), ldkv, N, tid);          // K and V loads in ONE round trip
    } else {
      df.load(da + prow * ldda + h * 64, half);
      stage_rows_f32<NT, 256>(reinterpret_cast<float*>(ks), kb, ldkv, N, tid);
      stage_rows_f32<NT, 256>(reinterpret_cast<float*>(vs), vb, ldkv, N, tid);
    }
    __syncthreads();
    RPO_STAMP(13);
    int l31v = l31;
    asm volatile("" : "+v"(l31v));
    // phase 1 (4 MFMAs per tile): row max and sum of the scores, online -- nothing else is kept, which keeps the
    // kernel at two workgroups per CU (all 384 (image, head) workgroups resident at once).  Each wave takes the key
    // tiles it will own in phase 2 (t = wave, wave + 4, ...); the four (max, sum) pairs are merged through 2 KB of LDS
    // behind the staging area (every wave scanning all tiles cost 6 k cycles of a 28 k-cycle kernel).
    float m = -INFINITY, l = 0.f;
#pragma unroll 1
    for (int t = wave; t < NT; t += 4) {
      f32x16_t sc = tile_times_frag<T>(ks, t, qf, l31v, half);
      const float mn = fmaxf(m, mask_and_max(sc, t, N, half));
      if (mn > -INFINITY) {                          // a wave whose tiles hold no key at all keeps (-inf, 0)
        l = l * exp_scalar<T>(m - mn, scale) + exp_tile<T>(sc, mn, scale);
        m = mn;
      }
    }
    l += __shfl_xor(l, 32, 64);
    float2* rowstat = reinterpret_cast<float2*>(smem + stat_off);   // [4 waves][64 lanes]
    rowstat[wave * 64 + lane] = make_float2(m, l);
    __syncthreads();
    {
      const float2 s0 = rowstat[lane], s1 = rowstat[64 + lane], s2 = rowstat[128 + lane], s3 = rowstat[192 + lane];
      m = fmaxf(fmaxf(s0.x, s1.x), fmaxf(s2.x, s3.x));              // tile 0 always holds keys: finite
      l = (s0.y * exp_scalar<T>(s0.x - m, scale) + s1.y * exp_scalar<T>(s1.x - m, scale)) +
          (s2.y * exp_scalar<T>(s2.x - m, scale) + s3.y * exp_scalar<T>(s3.x - m, scale));
    }
    const float inv = 1.0f / l;
    RPO_STAMP(14);
    // phase 2: this wave's key tiles t = wave, wave+4, ...
    f32x16_t u[2], w[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) { u[dt][r] = 0.f; w[dt][r] = 0.f; }
    float delta = 0.f;
#pragma unroll 1
    for (int t = wave; t < NT; t += 4) {           // wave-uniform trip count
      if constexpr (NCW > 0) bwd_pass2_tile<T, NT>(ks, vs, t, N, qf, dcd, m, inv, scale, u, w, delta, i0, i1, l31v, half);
      else bwd_pass2_tile<T, NT>(ks, vs, t, N, qf, df, m, inv, scale, u, w, delta, i0, i1, l31v, half);
    }
    delta += __shfl_xor(delta, 32, 64);
    RPO_STAMP(15);
    __syncthreads();                               // everybody is done with the staged K / V
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        part_u[(wave * 8 + dt * 4 + g) * 64 + lane] = make_float4(u[dt][4 * g], u[dt][4 * g + 1], u[dt][4 * g + 2], u[dt][4 * g + 3]);
        part_w[(wave * 8 + dt * 4 + g) * 64 + lane] = make_float4(w[dt][4 * g], w[dt][4 * g + 1], w[dt][4 * g + 2], w[dt][4 * g + 3]);
      }
    part_d[wave * 64 + lane] = delta;
    __syncthreads();
    const float dl = (part_d[lane] + part_d[64 + lane]) + (part_d[128 + lane] + part_d[192 + lane]);
    if (i < Kp) {
      T* orow = dq + prow * lddq + h * 64;
#pragma unroll
      for (int gg = 0; gg < 2; ++gg) {
        const int gi = wave * 2 + gg, dt = gi >> 2, g = gi & 3;
        float4 us = make_float4(0.f, 0.f, 0.f, 0.f), ws = us;
#pragma unroll
        for (int wv = 0; wv < 4; ++wv) {
          const float4 a = part_u[(wv * 8 + gi) * 64 + lane], c = part_w[(wv * 8 + gi) * 64 + lane];
          us.x += a.x; us.y += a.y; us.z += a.z; us.w += a.w;
          ws.x += c.x; ws.y += c.y; ws.z += c.z; ws.w += c.w;
        }
        ActIO<T>::st4(orow + 32 * dt + 8 * g + 4 * half, scale * (us.x - dl * ws.x), scale * (us.y - dl * ws.y),
                      scale * (us.z - dl * ws.z), scale * (us.w - dl * ws.w));
      }
    }
    RPO_STAMP(16);
  }
}

template <typename T, int NT, int NCW = 0>
__global__ __launch_bounds__(256, 2) void attn_bwd_kernel(const T* qr, int64_t ldq, const T* k, const T* v,
                                                       int64_t ldkv, const T* da, int64_t ldda,
                                                       T* dq, int64_t lddq, int B, int H, int N, int Kp,
                                                       float scale, const T* wo = nullptr, int64_t ldwo = 0,
                                                       const int32_t* key_len = nullptr, int key_stride = 0,
                                                       int nqt_wg = 1) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  attn_bwd_body<T, NT, NCW>(smem, blockIdx.x, gridDim.x, qr, ldq, k, v, ldkv, da, ldda, dq, lddq, B, H, N, Kp, scale, wo,
                            ldwo, key_len, key_stride, false, nqt_wg);
}

// Two attention-backward problems (d out-proj folded in) in one launch: workgroups [0, blocks0) are the (image, head)
// pairs of problem 0, the rest the (class, head) pairs of problem 1 -- the same stage of the two prompt-row chains.
struct AttnBwdProblem {
  const void* qr; int64_t ldq; const void* k; const void* v; int64_t ldkv; const void* da; int64_t ldda;
  void* dq; int64_t lddq; int B, H, N, Kp; float scale; const void* wo; int64_t ldwo; const int32_t* key_len; int key_stride;
};
// Problem 1 may get fewer workgroups than it has (group, head) items (each then walks items bid, bid + wgs1, ...): the
// kernel keeps two workgroups per CU resident, and a second round for a few dozen workgroups would double the launch.
template <typename T, int NT0, int NCW0, int NT1, int NCW1>
__global__ __launch_bounds__(256, 2) void attn_bwd_pair_kernel(const AttnBwdProblem a, const AttnBwdProblem b,
                                                            const int blocks0) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  if ((int)blockIdx.x < blocks0) {
    attn_bwd_body<T, NT0, NCW0>(smem, blockIdx.x, blocks0, static_cast<const T*>(a.qr), a.ldq, static_cast<const T*>(a.k),
                                static_cast<const T*>(a.v), a.ldkv, static_cast<const T*>(a.da), a.ldda,
                                static_cast<T*>(a.dq), a.lddq, a.B, a.H, a.N, a.Kp, a.scale, static_cast<const T*>(a.wo),
                                a.ldwo, a.key_len, a.key_stride);
  } else {
    const int items = b.B * b.H, first = (int)blockIdx.x - blocks0, wgs1 = (int)gridDim.x - blocks0;
    for (int t = first; t < items; t += wgs1) {
      if (t != first) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                           // the previous item's partials have been read
      }
      attn_bwd_body<T, NT1, NCW1>(smem, t, items, static_cast<const T*>(b.qr), b.ldq, static_cast<const T*>(b.k),
                                  static_cast<const T*>(b.v), b.ldkv, static_cast<const T*>(b.da), b.ldda,
                                  static_cast<T*>(b.dq), b.lddq, b.B, b.H, b.N, b.Kp, b.scale, static_cast<const T*>(b.wo),
                                  b.ldwo, b.key_len, b.key_stride);
    }
  }
}

// ---- long sequences (288 < N <= ATTN_LONG_MAX_N): the keys in chunks ------------------------------------------------------
// ViT-L/14 at 336 px has a 24 x 24 grid, N = 577: neither all keys of an image in LDS (about 165 KB of K rows and V^T
// fragments in the 16-bit modes) nor all score tiles of a query in registers fit.  These two kernels walk the keys in
// chunks of C = 32 LONG_NT = 256: a chunk is staged exactly as the kernels above stage all keys (16-bit: K rows padded
// to 144 B + V^T fragments transposed on the matrix core, 68 KB; f32: row-major [256][65] twice, 130 KB), consumed by every
// wave, and overwritten by the next one behind a barrier.  Keys past N inside the last chunk are staged as zeros and masked
// to -inf before the exponential: they contribute exact zeros.  Per query the arithmetic of a key tile is that of
// attn_fwd_kernel / attn_bwd_body; a lane holds one query, so a query's bits do not depend on its neighbours in the tile,
// on q_first or on the batch.
constexpr int LONG_NT = 8;
constexpr int ATTN_LONG_MAX_N = 1025;              // ViT-L/14 at 448 px (32 x 32 grid + CLS)

// Forward.  One workgroup per (image, head, group of 8 query tiles); a wave keeps ONE 32-query tile for the whole walk:
// its q fragment, running maximum, running sum and the fp32 output tile stay in registers across the chunks (online
// softmax), so nothing but K / V passes through LDS.  Each workgroup of an (image, head) stages the keys itself.
template <typename T>
__global__ __launch_bounds__(512, 4) void attn_fwd_long_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                            const T* __restrict__ v, int64_t ld, T* out, int64_t ldo,
                                                            int B, int H, int N, int Kp, float scale, int q_first,
                                                            int groups) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NT = LONG_NT, C = 32 * NT;
  using L = AL<T, NT>;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, l31 = lane & 31;
  const int unit = (int)blockIdx.x / groups, grp = (int)blockIdx.x - unit * groups;
  const int b = unit / H, h = unit % H;
  const T* kb = k + (int64_t)b * N * ld + h * 64;
  const T* vb = v + (int64_t)b * N * ld + h * 64;
  char* ks = smem;
  char* vs = smem + L::K_BYTES;
  const int S = N + Kp;
  // whole 32-query tiles before q_first are skipped, the leading queries of the first computed tile are not stored
  const int qt = (q_first >> 5) + 8 * grp + wave;
  const bool active = qt < ((S + 31) >> 5);        // wave-uniform; an idle wave still stages and meets the barriers
  const int s = qt * 32 + l31;
  const int64_t grow = frozen_prompt_row(s, b, B, N, Kp, S);
  RowFrag<T> qf;
  qf.load(q + grow * ld + h * 64, half);
  float m, l;
  f32x16_t o[2];
  fwd_reset(m, l, o);
#pragma unroll 1
  for (int c0 = 0; c0 < N; c0 += C) {
    const int Nc = min(N - c0, C);                 // keys of this chunk
    const T* kc = kb + (int64_t)c0 * ld;
    const T* vc = vb + (int64_t)c0 * ld;
    if (c0 > 0) __syncthreads();                   // the previous chunk has been consumed
    // (opaque copies: otherwise the staging addresses of every load are hoisted out of the chunk loop, kept live across
    //  the key loop and spilled)
    int tidv = tid, lanev = lane;
    asm volatile("" : "+v"(tidv), "+v"(lanev));
    const int l31s = lanev & 31, halfs = lanev >> 5;
    if constexpr (sizeof(T) == 2) {
      // K first, then V: with the query's state (q fragment, output tile) live across the chunks, both batches of loads
      // in flight at once do not fit 128 VGPRs
      stage_rows_bf16<NT, 512>(ks, reinterpret_cast<const bf16_t*>(kc), ld, Nc, tidv);
      asm volatile("" ::: "memory");
      VtRows<T, NT> vt;                            // wave w transposes key tile w of the chunk
      vt.load(vc, ld, Nc, wave, l31s, halfs);
      vt.park(vs, wave, lanev, l31s, halfs);
    } else {
      stage_rows_f32<NT, 512>(reinterpret_cast<float*>(ks), kc, ld, Nc, tidv);
      stage_rows_f32<NT, 512>(reinterpret_cast<float*>(vs), vc, ld, Nc, tidv);
    }
    __syncthreads();
    if (active) {
      int l31v = l31;                              // (opaque copy: see fwd_walk_keys)
      asm volatile("" : "+v"(l31v));
      // 16-bit: the chunk's full tiles, then its partial one (rem > 0: nfull < NT); f32: the tiles that hold a key, masked
      const int nt = sizeof(T) == 2 ? Nc >> 5 : (Nc + 31) >> 5;
      fwd_walk_keys<T, NT>(ks, vs, 0, nt, Nc & 31, Nc, qf, scale, m, l, o, l31v, half);
    }
  }
  fwd_store_tile<T>(out + grow * ldo + h * 64, o, l, active && s < S && s >= q_first, half);
}

// Backward for the prompt rows (dq; K and V are frozen).  One workgroup per (image, head, 32-query tile), the four waves
// sharing the tile as in attn_bwd_body: wave w owns key tiles w, w + 4 of EVERY chunk.  Pass 1 walks the chunks (K only)
// for the row maximum and sum -- per wave online over its tiles, merged once through LDS; pass 2 walks them again (K and V)
// and accumulates U, W and delta in registers across the chunks (for each chunk: stage, barrier, bwd_pass2_tile per key tile
// -- the step attn_bwd_body runs); the four waves' partials are summed through LDS in a fixed order.  No atomics: two calls
// give the same bits.
template <typename T>
__global__ __launch_bounds__(256, 2) void attn_bwd_long_kernel(const T* qr, int64_t ldq, const T* k, const T* v,
                                                            int64_t ldkv, const T* da, int64_t ldda, T* dq,
                                                            int64_t lddq, int B, int H, int N, int Kp, float scale,
                                                            int nqt) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NT = LONG_NT, C = 32 * NT;
  using L = AL<T, NT>;
  constexpr int stat_off = L::BWD_BYTES;           // the launcher allocates stat_off + 2048
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5, l31 = lane & 31;
  const int pair_id = (int)blockIdx.x / nqt, qt = (int)blockIdx.x - pair_id * nqt;
  const int b = pair_id / H, h = pair_id % H;
  const T* kb = k + (int64_t)b * N * ldkv + h * 64;
  const T* vb = v + (int64_t)b * N * ldkv + h * 64;
  char* ks = smem;
  char* vs = smem + L::K_BYTES;
  float4* part_u = reinterpret_cast<float4*>(smem);                 // [4 waves][8 groups][64 lanes]
  float4* part_w = part_u + 4 * 8 * 64;
  float* part_d = reinterpret_cast<float*>(part_w + 4 * 8 * 64);    // [4 waves][64 lanes]
  bf16x8_t i0, i1;
  if constexpr (sizeof(T) == 2) { i0 = ident_frag<T>(0, l31, half); i1 = ident_frag<T>(1, l31, half); }
  const int i = qt * 32 + l31;
  const int64_t prow = (int64_t)b * Kp + min(i, Kp - 1);
  RowFrag<T> qf, df;
  qf.load(qr + prow * ldq + h * 64, half);
  df.load(da + prow * ldda + h * 64, half);

  // pass 1: row maximum and sum
  float m = -INFINITY, l = 0.f;
#pragma unroll 1
  for (int c0 = 0; c0 < N; c0 += C) {
    const int Nc = min(N - c0, C);
    if (c0 > 0) __syncthreads();
    if constexpr (sizeof(T) == 2)
      stage_rows_bf16<NT, 256>(ks, reinterpret_cast<const bf16_t*>(kb + (int64_t)c0 * ldkv), ldkv, Nc, tid);
    else
      stage_rows_f32<NT, 256>(reinterpret_cast<float*>(ks), kb + (int64_t)c0 * ldkv, ldkv, Nc, tid);
    __syncthreads();
    int l31v = l31;
    asm volatile("" : "+v"(l31v));
#pragma unroll 1
    for (int t = wave; 32 * t < Nc; t += 4) {      // every tile visited holds a key: mn is finite
      f32x16_t sc = tile_times_frag<T>(ks, t, qf, l31v, half);
      const float mn = fmaxf(m, mask_and_max(sc, t, Nc, half));
      l = l * exp_scalar<T>(m - mn, scale) + exp_tile<T>(sc, mn, scale);
      m = mn;
    }
  }
  l += __shfl_xor(l, 32, 64);
  float2* rowstat = reinterpret_cast<float2*>(smem + stat_off);     // [4 waves][64 lanes], behind the staging area
  rowstat[wave * 64 + lane] = make_float2(m, l);
  __syncthreads();                                 // also: everybody is done with the last chunk of pass 1
  {
    const float2 s0 = rowstat[lane], s1 = rowstat[64 + lane], s2 = rowstat[128 + lane], s3 = rowstat[192 + lane];
    m = fmaxf(fmaxf(s0.x, s1.x), fmaxf(s2.x, s3.x));                // N > 288: every wave has seen keys
    l = (s0.y * exp_scalar<T>(s0.x - m, scale) + s1.y * exp_scalar<T>(s1.x - m, scale)) +
        (s2.y * exp_scalar<T>(s2.x - m, scale) + s3.y * exp_scalar<T>(s3.x - m, scale));
  }
  const float inv = 1.0f / l;

  // pass 2: dP, delta, U = sum (p dp) K, W = sum p K
  f32x16_t u[2], w[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) { u[dt][r] = 0.f; w[dt][r] = 0.f; }
  float delta = 0.f;
#pragma unroll 1
  for (int c0 = 0; c0 < N; c0 += C) {
    const int Nc = min(N - c0, C);
    if (c0 > 0) __syncthreads();
    if constexpr (sizeof(T) == 2) {
      stage2_bf16<NT, 256>(ks, vs, reinterpret_cast<const bf16_t*>(kb + (int64_t)c0 * ldkv),
                           reinterpret_cast<const bf16_t*>(vb + (int64_t)c0 * ldkv), ldkv, Nc, tid);
    } else {
      stage_rows_f32<NT, 256>(reinterpret_cast<float*>(ks), kb + (int64_t)c0 * ldkv, ldkv, Nc, tid);
      stage_rows_f32<NT, 256>(reinterpret_cast<float*>(vs), vb + (int64_t)c0 * ldkv, ldkv, Nc, tid);
    }
    __syncthreads();
    int l31v = l31;
    asm volatile("" : "+v"(l31v));
#pragma unroll 1
    for (int t = wave; 32 * t < Nc; t += 4) {      // wave-uniform trip count
      bwd_pass2_tile<T, NT>(ks, vs, t, Nc, qf, df, m, inv, scale, u, w, delta, i0, i1, l31v, half);
    }
  }
  delta += __shfl_xor(delta, 32, 64);
  __syncthreads();                                 // everybody is done with the staged K / V
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      part_u[(wave * 8 + dt * 4 + g) * 64 + lane] = make_float4(u[dt][4 * g], u[dt][4 * g + 1], u[dt][4 * g + 2], u[dt][4 * g + 3]);
      part_w[(wave * 8 + dt * 4 + g) * 64 + lane] = make_float4(w[dt][4 * g], w[dt][4 * g + 1], w[dt][4 * g + 2], w[dt][4 * g + 3]);
    }
  part_d[wave * 64 + lane] = delta;
  __syncthreads();
  const float dl = (part_d[lane] + part_d[64 + lane]) + (part_d[128 + lane] + part_d[192 + lane]);
  if (i < Kp) {
    T* orow = dq + prow * lddq + h * 64;
#pragma unroll
    for (int gg = 0; gg < 2; ++gg) {
      const int gi = wave * 2 + gg, dt = gi >> 2, g = gi & 3;
      float4 us = make_float4(0.f, 0.f, 0.f, 0.f), ws = us;
#pragma unroll
      for (int wv = 0; wv < 4; ++wv) {
        const float4 a = part_u[(wv * 8 + gi) * 64 + lane], c = part_w[(wv * 8 + gi) * 64 + lane];
        us.x += a.x; us.y += a.y; us.z += a.z; us.w += a.w;
        ws.x += c.x; ws.y += c.y; ws.z += c.z; ws.w += c.w;
      }
      ActIO<T>::st4(orow + 32 * dt + 8 * g + 4 * half, scale * (us.x - dl * ws.x), scale * (us.y - dl * ws.y),
                    scale * (us.z - dl * ws.z), scale * (us.w - dl * ws.w));
    }
  }
}

template <typename T>
int launch_fwd_long(const void* q, const void* k, const void* v, int64_t ld, void* out, int64_t ldo, int B, int H,
                    int N, int Kp, float scale, int q_first, hipStream_t s) {
  static rpo_lds_mask_t lds_ok{0};
  auto kern = attn_fwd_long_kernel<T>;
  constexpr int bytes = AL<T, LONG_NT>::FWD_BYTES;
  if (int rc = rpo_allow_lds(reinterpret_cast<const void*>(kern), bytes, &lds_ok)) return rc;
  const int tiles = ((N + Kp + 31) >> 5) - (q_first >> 5), groups = (tiles + 7) / 8;
  if ((int64_t)B * H * groups > INT32_MAX) return RPO_E_SHAPE;
  hipLaunchKernelGGL(kern, dim3(B * H * groups), dim3(512), bytes, s, static_cast<const T*>(q), static_cast<const T*>(k),
                     static_cast<const T*>(v), ld, static_cast<T*>(out), ldo, B, H, N, Kp, scale, q_first, groups);
  return rpo_launch_status();
}

template <typename T>
int launch_bwd_long(const void* qr, int64_t ldq, const void* k, const void* v, int64_t ldkv, const void* da,
                    int64_t ldda, void* dq, int64_t lddq, int B, int H, int N, int Kp, float scale, hipStream_t s) {
  static rpo_lds_mask_t lds_ok{0};
  auto kern = attn_bwd_long_kernel<T>;
  constexpr int bytes = AL<T, LONG_NT>::BWD_BYTES + 2048;
  if (int rc = rpo_allow_lds(reinterpret_cast<const void*>(kern), bytes, &lds_ok)) return rc;
  const int nqt = (Kp + 31) / 32;
  if ((int64_t)B * H * nqt > INT32_MAX) return RPO_E_SHAPE;
  hipLaunchKernelGGL(kern, dim3(B * H * nqt), dim3(256), bytes, s, static_cast<const T*>(qr), ldq,
                     static_cast<const T*>(k), static_cast<const T*>(v), ldkv, static_cast<const T*>(da), ldda,
                     static_cast<T*>(dq), lddq, B, H, N, Kp, scale, nqt);
  return rpo_launch_status();
}

template <typename T, int NT>
int launch_fwd(const void* q, const void* k, const void* v, int64_t ld, void* out, int64_t ldo, int B, int H,
               int N, int Kp, float scale, int q_first, hipStream_t s) {
  // round 6: two-phase staging where the launch has more (image, head) units than CUs and seven key tiles (ViT-B/16 from
  // batch 22 on) -- there the staging burst is long and the early start pays (batch 64: -0.5 % on the step); with fewer
  // units (or ViT-L/14's nine key tiles, 256 units at batch 16) the second barrier's wave skew costs more than the early start
  // returns (ViT-L/14 +0.8 %): profiles/r06_ab_attn_configs.txt.
  const bool two_phase = NT == 7 && B * H > rpo_cu_count();
  if constexpr (sizeof(T) == 2) if (two_phase) {
    static rpo_lds_mask_t lds16_ok{0};
    auto k16 = attn_fwd16_kernel<T, NT>;
    constexpr int bytes16 = AL16<T, NT>::BYTES;
    if (int rc = rpo_allow_lds(reinterpret_cast<const void*>(k16), bytes16, &lds16_ok)) return rc;
    hipLaunchKernelGGL(k16, dim3(B * H), dim3(512), bytes16, s, static_cast<const T*>(q), static_cast<const T*>(k),
                       static_cast<const T*>(v), ld, static_cast<T*>(out), ldo, B, H, N, Kp, scale, q_first);
    return rpo_launch_status();
  }
  static rpo_lds_mask_t lds_ok{0};
  auto kern = attn_fwd_kernel<T, NT>;
  constexpr int bytes = AL<T, NT>::FWD_BYTES;
  if (int rc = rpo_allow_lds(reinterpret_cast<const void*>(kern), bytes, &lds_ok)) return rc;
  hipLaunchKernelGGL(kern, dim3(B * H), dim3(512), bytes, s, static_cast<const T*>(q), static_cast<const T*>(k),
                     static_cast<const T*>(v), ld, static_cast<T*>(out), ldo, B, H, N, Kp, scale, q_first);   // two workgroups fit a CU
  return rpo_launch_status();
}

// ---- forward, prompt queries of SEVERAL prompt sets over one image's frozen K / V (rpo_attn_prompt_fwd) -----------------
// The prompt rows of `sets` prompt sets, each a batch of B images x Kp queries in buffers of their own (set-major: row
// (s B + b) Kp + j), read the frozen K / V of image first + b: rows (first + b) N ... of k / v, which lie in the live
// packed in-proj output of the frozen pass (ldkv = 3 d) or in a cache of it (ldkv = 2 d).  One workgroup per (image, head)
// stages that image's K / V once -- exactly as attn_fwd_kernel does: K rows padded to 144 B, V^T fragments transposed on
// the matrix core (16-bit); row-major [NPAD][65] (f32) -- and then serves the sets * Kp queries of the image as 32-query
// tiles, one wave each.  A lane holds ONE query (S^T = K . Q^T), so the queries of a tile may belong to different sets and
// a query's result does not depend on which other queries share its tile: set s of a launch is bit for bit the launch of
// that set alone.  Per query the arithmetic is attn_fwd_kernel's (online softmax in fp32, P rounded to the storage type
// for P.V in the 16-bit modes, fp32 P on the 32x32x2 f32 MFMA in the f32 mode).
// `first` is read on the device: a captured graph serves every chunk of a cached set.
template <typename T, int NT>
__global__ __launch_bounds__(512, 4) void attn_prompt_fwd_kernel(const T* __restrict__ q, int64_t ldq,
                                                              const T* __restrict__ k, const T* __restrict__ v,
                                                              int64_t ldkv, T* out, int64_t ldo, int B, int H, int N,
                                                              int Kp, int sets, const int32_t* __restrict__ first,
                                                              float scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using L = AL<T, NT>;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, l31 = lane & 31;
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const int64_t img = (int64_t)(first != nullptr ? *first : 0) + b;
  const T* kb = k + img * N * ldkv + h * 64;
  const T* vb = v + img * N * ldkv + h * 64;
  char* ks = smem;
  char* vs = smem + L::K_BYTES;
  const int Q = sets * Kp;                               // this image's queries, set-major
  const int qt_end = (Q + 31) >> 5;
  // (queries past Q: the last one again, computed and not stored)
  auto qrow = [&](int qt) { return set_major_row(qt * 32 + l31, b, B, Kp, Q); };
  RowFrag<T> qf;
  if constexpr (sizeof(T) == 2) qf.load(q + qrow(wave) * ldq + h * 64, half);
  if constexpr (sizeof(T) == 2) {
    VtRows<T, NT> vt;
    vt.load(vb, ldkv, N, wave, l31, half);
    stage_rows_bf16<NT, 512>(ks, reinterpret_cast<const bf16_t*>(kb), ldkv, N, tid);
    vt.park(vs, wave, lane, l31, half);
  } else {
    stage_rows_f32<NT, 512>(reinterpret_cast<float*>(ks), kb, ldkv, N, tid);
    stage_rows_f32<NT, 512>(reinterpret_cast<float*>(vs), vb, ldkv, N, tid);
  }
  __syncthreads();
  const int nfull = sizeof(T) == 2 ? min(N >> 5, NT) : NT, rem = nfull < NT ? N - 32 * nfull : 0;   // (as attn_fwd_kernel)
  for (int qt = wave; qt < qt_end; qt += 8) {
    int l31v = l31;                                      // (opaque copy: see fwd_walk_keys)
    asm volatile("" : "+v"(l31v));
    const int64_t grow = qrow(qt);
    if (sizeof(T) != 2 || qt != wave) qf.load(q + grow * ldq + h * 64, half);
    float m, l;
    f32x16_t o[2];
    fwd_reset(m, l, o);
    fwd_walk_keys<T, NT>(ks, vs, 0, nfull, rem, N, qf, scale, m, l, o, l31v, half);
    fwd_store_tile<T>(out + grow * ldo + h * 64, o, l, qt * 32 + l31 < Q, half);
  }
}

template <typename T, int NT>
int launch_prompt_fwd(const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, void* out, int64_t ldo,
                      int B, int H, int N, int Kp, int sets, const int32_t* first, float scale, hipStream_t s) {
  static rpo_lds_mask_t lds_ok{0};
  auto kern = attn_prompt_fwd_kernel<T, NT>;
  constexpr int bytes = AL<T, NT>::FWD_BYTES;
  if (int rc = rpo_allow_lds(reinterpret_cast<const void*>(kern), bytes, &lds_ok)) return rc;
  hipLaunchKernelGGL(kern, dim3(B * H), dim3(512), bytes, s, static_cast<const T*>(q), ldq, static_cast<const T*>(k),
                     static_cast<const T*>(v), ldkv, static_cast<T*>(out), ldo, B, H, N, Kp, sets, first, scale);
  return rpo_launch_status();
}

// ---- backward, prompt queries of SEVERAL prompt sets over one image's frozen K / V (rpo_attn_prompt_bwd) ----------------
// The backward twin of attn_prompt_fwd_kernel, same row layout (set-major: row (s B + b) Kp + j) and the same `first`:
// dq = scale * (U - delta W) as attn_bwd_body defines it, P recomputed from q and K, nothing saved by the forward, no dK / dV
// (the keys and values belong to frozen tokens).  One workgroup of eight waves per (image, head) stages that image's K and V
// row-major ONCE (16-bit: rows padded to 144 B, 2 x K_BYTES = 82 944 B at NT = 9; f32: [NPAD][65] floats twice, 149 760 B)
// and serves the sets * Kp queries of the image as 32-query tiles.
// Shape, ALL storage types: one wave walks ALL key tiles of its own query tile -- twice: the row maximum, the row sum and
// delta = sum P o dP online, then dS = P o (dP - delta) and its contraction with K -- so everything of a query is complete in
// the wave's registers.  dS . K IS U - delta W; with delta known before the contraction the 16-bit modes round P o (dP - delta)
// ONCE instead of rounding P o dP and P separately and cancelling U against delta W afterwards (that arrangement measured
// 2.97e-3 of the reference's maximum in f16 at N = 5, Kp = 1, outside the op-level bound of 2e-3), and W's accumulators and
// MFMAs are not needed: the second dP product of pass 1 costs what W's contraction cost.  attn_bwd_body instead spreads the key
// tiles of ONE query tile over four waves and combines their partials (66 560 B) through the dead staging area; here the
// staging must stay live across the query tiles.  In the 16-bit modes the partials would fit beside it (149 504 B), in f32 at
// NT = 9 they do not, and with the query tiles of several sets to hand out the waves are busy without splitting a tile:
// no partials, no barrier after the staging one, one code path for the three storage types.  (One set of Kp <= 32 is one
// busy wave per workgroup: the single-set step keeps rpo_attn_readonly_bwd.)
// A lane holds ONE query (S^T = K . Q^T; the columns of every MFMA here are queries), the key loop's trip count depends on N
// alone and no branch looks at another lane's data: a query's bits depend neither on `sets`, nor on its position in a tile,
// nor on its neighbours -- set s of a launch is bit for bit the launch of that set alone.  Fixed summation order (key tiles
// ascending), no atomics.
template <typename T, int NT>
__global__ __launch_bounds__(512) void attn_prompt_bwd_kernel(const T* q, int64_t ldq, const T* k, const T* v, int64_t ldkv,
                                                           const T* da, int64_t ldda, T* dq, int64_t lddq, int B, int H,
                                                           int N, int Kp, int sets, const int32_t* first, float scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using L = AL<T, NT>;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5, l31 = lane & 31;
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const int64_t img = (int64_t)(first != nullptr ? *first : 0) + b;
  const T* kb = k + img * N * ldkv + h * 64;
  const T* vb = v + img * N * ldkv + h * 64;
  char* ks = smem;
  char* vs = smem + L::K_BYTES;
  const int Q = sets * Kp;                               // this image's queries, set-major
  const int qt_end = (Q + 31) >> 5;
  // (queries past Q: the last one again, computed and not stored)
  auto qrow = [&](int qt) { return set_major_row(qt * 32 + l31, b, B, Kp, Q); };
  RowFrag<T> qf, df;
  if constexpr (sizeof(T) == 2) {                        // the first tile's operands ride in the staging loads' round trip
    const int64_t r0 = qrow(wave);
    qf.load(q + r0 * ldq + h * 64, half);
    df.load(da + r0 * ldda + h * 64, half);
    stage2_bf16<NT, 512>(ks, vs, reinterpret_cast<const bf16_t*>(kb), reinterpret_cast<const bf16_t*>(vb), ldkv, N, tid);
  } else {
    stage_rows_f32<NT, 512>(reinterpret_cast<float*>(ks), kb, ldkv, N, tid);
    stage_rows_f32<NT, 512>(reinterpret_cast<float*>(vs), vb, ldkv, N, tid);
  }
  __syncthreads();                                       // the only barrier: K / V are read-only from here on
  bf16x8_t i0, i1;
  if constexpr (sizeof(T) == 2) { i0 = ident_frag<T>(0, l31, half); i1 = ident_frag<T>(1, l31, half); }
  const int nkt = min(NT, (N + 31) >> 5);                // key tiles that hold a key (rows past N are staged as zeros)
  for (int qt = wave; qt < qt_end; qt += 8) {
    int l31v = l31;                                      // (keeps the K / V ds_reads inside the loops: attn_fwd_kernel)
    asm volatile("" : "+v"(l31v));
    const int vq = qt * 32 + l31;
    const int64_t grow = qrow(qt);
    if (sizeof(T) != 2 || qt != wave) {
      qf.load(q + grow * ldq + h * 64, half);
      df.load(da + grow * ldda + h * 64, half);
    }
    // pass 1: row maximum, sum of the scores and delta = sum P o dP (dP = da . V^T), online over the key tiles in ascending order
    float m = -INFINITY, l = 0.f, dsum = 0.f;
#pragma unroll 1
    for (int t = 0; t < nkt; ++t) {
      f32x16_t sc = tile_times_frag<T>(ks, t, qf, l31v, half);
      const f32x16_t dp = tile_times_frag<T>(vs, t, df, l31v, half);   // (V rows past N are zeros: finite)
      const float mn = fmaxf(m, mask_and_max(sc, t, N, half));     // finite from tile 0 on (N >= 1)
      const float alpha = exp_scalar<T>(m - mn, scale);            // first tile: exp(-inf) = 0
      l = l * alpha + exp_tile<T>(sc, mn, scale);
      float dt_ = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) dt_ = fmaf(sc[r], dp[r], dt_);  // (exp = 0 on padded keys)
      dsum = dsum * alpha + dt_;
      m = mn;
    }
    l += __shfl_xor(l, 32, 64);
    dsum += __shfl_xor(dsum, 32, 64);
    const float inv = 1.0f / l;
    const float delta = dsum * inv;
    // pass 2: dS = P o (dP - delta) in fp32, rounded ONCE to the storage type (16-bit modes), and U' = dS . K
    f32x16_t u[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) u[dt][r] = 0.f;
#pragma unroll 1
    for (int t = 0; t < nkt; ++t) {
      f32x16_t pt = tile_times_frag<T>(ks, t, qf, l31v, half);
      (void)mask_and_max(pt, t, N, half);
      (void)exp_tile<T>(pt, m, scale);
      const f32x16_t dp = tile_times_frag<T>(vs, t, df, l31v, half);
      if constexpr (sizeof(T) == 2) {
        const char* krow = ks + (32 * t + l31v) * 144 + half * 16;
        bf16x8_t krows[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) krows[kk] = *reinterpret_cast<const bf16x8_t*>(krow + kk * 32);
        float ds[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) ds[r] = (pt[r] * inv) * (dp[r] - delta);   // (P = 0 on padded keys)
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          bf16x8_t ktf[2];
          transpose_tile<T>(krows, dt, i0, i1, ktf);     // K^T fragments of this key tile, in registers
#pragma unroll
          for (int g2 = 0; g2 < 2; ++g2) u[dt] = mfma16<T>(ktf[g2], pack8<T>(ds + 8 * g2), u[dt]);
        }
      } else {
        f32x16_t ds;
#pragma unroll
        for (int r = 0; r < 16; ++r) ds[r] = (pt[r] * inv) * (dp[r] - delta);
        contract_keys<T, NT>(ks, t, ds, u, l31v, half);
      }
    }
    if (vq < Q) store_tile<T>(dq + grow * lddq + h * 64, u, scale, half);
  }
}

template <typename T, int NT>
int launch_prompt_bwd(const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, const void* da, int64_t ldda,
                      void* dq, int64_t lddq, int B, int H, int N, int Kp, int sets, const int32_t* first, float scale,
                      hipStream_t s) {
  static rpo_lds_mask_t lds_ok{0};
  auto kern = attn_prompt_bwd_kernel<T, NT>;
  constexpr int bytes = AL<T, NT>::BWD_STAGE;
  if (int rc = rpo_allow_lds(reinterpret_cast<const void*>(kern), bytes, &lds_ok)) return rc;
  hipLaunchKernelGGL(kern, dim3(B * H), dim3(512), bytes, s, static_cast<const T*>(q), ldq, static_cast<const T*>(k),
                     static_cast<const T*>(v), ldkv, static_cast<const T*>(da), ldda, static_cast<T*>(dq), lddq, B, H, N, Kp,
                     sets, first, scale);
  return rpo_launch_status();
}

// dynamic LDS of attn_bwd_kernel<T, NT, NCW>: the staging area / the partials -- NCW > 0: or the 4 waves x 2 (NCW = 4: 4)
// weight slots of 8 KiB that the folded out-proj lands in first -- and 2 KB of row statistics behind them
constexpr int bwd_lds(int bwd_bytes, int ncw) {
  const int slots = ncw == 0 ? 0 : 4 * (ncw == 4 ? 4 : 2) * 8192;
  return (bwd_bytes > slots ? bwd_bytes : slots) + 2048;
}

bool ok_ld(int64_t ld, int esz) { return (ld * esz) % 16 == 0; }

// The one launcher of attn_bwd_kernel: nqt_wg workgroups per (group, head), one per 32-query tile (NCW > 0 with Kp > 32),
// or one that walks the query tiles itself (nqt_wg = 1).  a.key_len: per-group key counts (the text tower).
template <typename T, int NT, int NCW = 0>
int launch_bwd(const AttnBwdProblem& a, int nqt_wg, hipStream_t s) {
  static rpo_lds_mask_t lds_ok{0};
  auto kern = attn_bwd_kernel<T, NT, NCW>;
  constexpr int bytes = bwd_lds(AL<T, NT>::BWD_BYTES, NCW);
  if (int rc = rpo_allow_lds(reinterpret_cast<const void*>(kern), bytes, &lds_ok)) return rc;
  hipLaunchKernelGGL(kern, dim3(a.B * a.H * nqt_wg), dim3(256), bytes, s, static_cast<const T*>(a.qr), a.ldq,
                     static_cast<const T*>(a.k), static_cast<const T*>(a.v), a.ldkv, static_cast<const T*>(a.da), a.ldda,
                     static_cast<T*>(a.dq), a.lddq, a.B, a.H, a.N, a.Kp, a.scale, static_cast<const T*>(a.wo), a.ldwo,
                     a.key_len, a.key_stride, nqt_wg);
  return rpo_launch_status();
}
template <typename T, int NT0, int NCW0, int NT1, int NCW1>
int launch_bwd_proj_pair(const AttnBwdProblem& a, const AttnBwdProblem& b, hipStream_t s) {
  static rpo_lds_mask_t lds_ok{0};
  auto kern = attn_bwd_pair_kernel<T, NT0, NCW0, NT1, NCW1>;
  constexpr int b0 = bwd_lds(AL<T, NT0>::BWD_BYTES, NCW0), b1 = bwd_lds(AL<T, NT1>::BWD_BYTES, NCW1);
  constexpr int bytes = b0 > b1 ? b0 : b1;
  if (int rc = rpo_allow_lds(reinterpret_cast<const void*>(kern), bytes, &lds_ok)) return rc;
  const int items0 = a.B * a.H, items1 = b.B * b.H, slots = 2 * rpo_cu_count();
  int wgs1 = items1;
  for (int walk = 2; items0 + wgs1 > slots && walk <= 8; ++walk) wgs1 = (items1 + walk - 1) / walk;
  hipLaunchKernelGGL(kern, dim3(items0 + wgs1), dim3(256), bytes, s, a, b, items0);
  return rpo_launch_status();
}
// (key tiles, 256-column chunks of d) of one problem; 0 if the fused kernel does not cover it
inline int bwd_proj_geometry(const rpo_attn_bwd_args& a, int* nt, int* ncw) {
  const int d = a.H * 64;
  if (a.keys > 288 || a.Kp > 32 || (d != 512 && d != 768)) return 0;
  *nt = a.keys <= 96 ? 3 : (a.keys <= 224 ? 7 : 9);
  *ncw = d / 256;
  return 1;
}
inline int bwd_proj_check(const rpo_attn_bwd_args& a) {
  if (!a.q_rows || !a.k || !a.v || !a.dx || !a.w_out_t || !a.dq || a.groups <= 0 || a.H <= 0 || a.keys <= 0 || a.Kp <= 0)
    return RPO_E_BADARG;
  if (a.key_len != nullptr && a.key_stride < a.keys) return RPO_E_BADARG;
  if (!aligned16(a.q_rows) || !aligned16(a.k) || !aligned16(a.v) || !aligned16(a.dx) || !aligned16(a.w_out_t) ||
      !ok_ld(a.ldq, 2) || !ok_ld(a.ldkv, 2) || !ok_ld(a.lddx, 2) || !ok_ld(a.ldw, 2) ||
      reinterpret_cast<uintptr_t>(a.dq) % 8 || (a.lddq * 2) % 8) return RPO_E_ALIGN;
  return 0;
}
inline AttnBwdProblem bwd_problem(const rpo_attn_bwd_args& a) {
  return AttnBwdProblem{a.q_rows, a.ldq, a.k, a.v, a.ldkv, a.dx, a.lddx, a.dq, a.lddq, a.groups, a.H, a.keys, a.Kp,
                        a.scale, a.w_out_t, a.ldw, a.key_len, a.key_len ? a.key_stride : a.keys};
}
template <typename T>
int dispatch_bwd_proj_args(const rpo_attn_bwd_args* a0, const rpo_attn_bwd_args* a1, hipStream_t s) {
  int nt0, ncw0, nt1 = 0, ncw1 = 0;
  if (!bwd_proj_geometry(*a0, &nt0, &ncw0) || (a1 && !bwd_proj_geometry(*a1, &nt1, &ncw1))) return RPO_E_SHAPE;
  const AttnBwdProblem p0 = bwd_problem(*a0);
  if (a1 == nullptr) {
#define RPO_BV(NT_, NCW_) if (nt0 == NT_ && ncw0 == NCW_) return launch_bwd<T, NT_, NCW_>(p0, 1, s)
    RPO_BV(3, 2); RPO_BV(3, 3); RPO_BV(7, 2); RPO_BV(7, 3); RPO_BV(9, 2); RPO_BV(9, 3);
#undef RPO_BV
    return RPO_E_SHAPE;
  }
  const AttnBwdProblem p1 = bwd_problem(*a1);
  // the pairs a step of this repo's models forms: image tower (197 keys, d 768) with the text tower (<= 96 keys, d 512)
#define RPO_BPAIR(A, B, C, D) if (nt0 == A && ncw0 == B && nt1 == C && ncw1 == D) return launch_bwd_proj_pair<T, A, B, C, D>(p0, p1, s)
  RPO_BPAIR(7, 3, 3, 2);
  RPO_BPAIR(7, 3, 3, 3);
#undef RPO_BPAIR
  return RPO_E_SHAPE;
}
template <typename T>
int dispatch_bwd_proj(int ncw, bool big, const AttnBwdProblem& a, hipStream_t s) {
  const int nqt = (a.Kp + 31) / 32;                // one workgroup per (image, head, 32-query tile)
#define RPO_BP(NT_, NCW_) return launch_bwd<T, NT_, NCW_>(a, nqt, s)
  if (ncw == 2) { if (big) RPO_BP(9, 2); RPO_BP(7, 2); }
  if (ncw == 3) { if (big) RPO_BP(9, 3); RPO_BP(7, 3); }
  if (ncw == 4) { if (big) RPO_BP(9, 4); RPO_BP(7, 4); }
#undef RPO_BP
  return RPO_E_SHAPE;
}


// ---- text tower, prompt rows (round 5): one WAVE per (class, head) -------------------------------------------------------
// The prompt rows of a class read only that class's frozen tokens (trainers/rpo.py:144-151): K <= 64 queries against
// len_c keys -- 8 .. 14 for the Oxford-Pets prompts, <= 77 for any CLIP prompt -- per (class, head).  That is one or two
// 32x32 MFMA tiles, so a single wave holds the whole problem in registers: K and V rows come straight from the row-major
// K / V cache as A-operand fragments (16 B per lane), S^T = K . Q^T leaves a lane with ONE query's scores (softmax =
// in-register reduce + one cross-half exchange), V^T / K^T for the second contraction are formed on the matrix core
// (transpose_tile: exact), P / dS go from the C/D registers straight into the B operand.  No LDS, no barrier, 64 threads.
// It replaces the VALU kernel of attn_text.hip (912 workgroups of 256 threads for the same work) in the 16-bit modes.
//   forward : out = softmax(scale q K^T) V                                      (clip/model.py:186 under the mask above)
//   backward: dq = scale * sum_key dS[key] K[key],  dS = P (dP - sum P dP),  dP = da V^T   (K, V frozen: no dK, dV)
template <typename T, bool BWD, int NKT>
__global__ __launch_bounds__(64) void text_attn_wave_kernel(const T* q, int64_t ldq, const T* kc, const T* vc, int64_t ldkv,
                                                            const T* da, int64_t ldda, T* out, int64_t ldo,
                                                            const int32_t* __restrict__ len, int rows, int Lmax, int H,
                                                            float scale, int n_kv) {
  const int lane = threadIdx.x, half = lane >> 5, l31 = lane & 31;
  const int c = blockIdx.x / H, h = blockIdx.x % H;
  const int ckv = c % n_kv;                // the cached class this (virtual) class reads: c itself when n_kv = n_cls
  const int L = min(len[ckv], Lmax);
  RowFrag<T> kf[NKT], vf[NKT];
#pragma unroll
  for (int t = 0; t < NKT; ++t) {          // keys >= L: the last key again (scores masked, p = 0 exactly)
    const int64_t base = ((int64_t)ckv * Lmax + max(min(32 * t + l31, L - 1), 0)) * ldkv + h * 64;
    kf[t].load(kc + base, half);
    vf[t].load(vc + base, half);
  }
  const bf16x8_t i0 = ident_frag<T>(0, l31, half), i1 = ident_frag<T>(1, l31, half);
  for (int r0 = 0; r0 < rows; r0 += 32) {
    const int r = r0 + l31;
    const int64_t row = (int64_t)c * rows + min(r, rows - 1);
    RowFrag<T> qf, df;
    qf.load(q + row * ldq + h * 64, half);
    if constexpr (BWD) df.load(da + row * ldda + h * 64, half);
    f32x16_t s[NKT];
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < NKT; ++t) {
#pragma unroll
      for (int e = 0; e < 16; ++e) s[t][e] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) s[t] = mfma16<T>(kf[t].f[ks], qf.f[ks], s[t]);
      m = fmaxf(m, mask_and_max(s[t], t, L, half));
    }
    float l = 0.f;
#pragma unroll
    for (int t = 0; t < NKT; ++t) l += exp_tile<T>(s[t], m, scale);
    l += __shfl_xor(l, 32, 64);
    const float inv = 1.0f / l;
    f32x16_t o[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int e = 0; e < 16; ++e) o[dt][e] = 0.f;
    float fin = inv;
    if constexpr (!BWD) {
#pragma unroll
      for (int t = 0; t < NKT; ++t) {
        float w[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) w[e] = s[t][e];
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          bf16x8_t vt[2];
          transpose_tile<T>(vf[t].f, dt, i0, i1, vt);
#pragma unroll
          for (int g2 = 0; g2 < 2; ++g2) o[dt] = mfma16<T>(vt[g2], pack8<T>(w + 8 * g2), o[dt]);
        }
      }
    } else {
      f32x16_t dp[NKT];
      float delta = 0.f;
#pragma unroll
      for (int t = 0; t < NKT; ++t) {
#pragma unroll
        for (int e = 0; e < 16; ++e) dp[t][e] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) dp[t] = mfma16<T>(vf[t].f[ks], df.f[ks], dp[t]);
#pragma unroll
        for (int e = 0; e < 16; ++e) { s[t][e] *= inv; delta = fmaf(s[t][e], dp[t][e], delta); }
      }
      delta += __shfl_xor(delta, 32, 64);
#pragma unroll
      for (int t = 0; t < NKT; ++t) {
        float w[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) w[e] = s[t][e] * (dp[t][e] - delta);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          bf16x8_t kt[2];
          transpose_tile<T>(kf[t].f, dt, i0, i1, kt);
#pragma unroll
          for (int g2 = 0; g2 < 2; ++g2) o[dt] = mfma16<T>(kt[g2], pack8<T>(w + 8 * g2), o[dt]);
        }
      }
      fin = scale;
    }
    if (r < rows) {
      T* orow = out + row * ldo + h * 64;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          ActIO<T>::st4(orow + 32 * dt + 8 * g + 4 * half, o[dt][4 * g] * fin, o[dt][4 * g + 1] * fin,
                        o[dt][4 * g + 2] * fin, o[dt][4 * g + 3] * fin);
    }
  }
}

template <typename T, bool BWD>
int launch_text_wave(const void* q, int64_t ldq, const void* kc, const void* vc, int64_t ldkv, const void* da, int64_t ldda,
                     void* out, int64_t ldo, const int32_t* len, int n_cls, int n_kv, int rows, int Lmax, int H, float scale,
                     hipStream_t s) {
#define RPO_TW(NKT)                                                                                                   \
  hipLaunchKernelGGL((text_attn_wave_kernel<T, BWD, NKT>), dim3(n_cls * H), dim3(64), 0, s, static_cast<const T*>(q), \
                     ldq, static_cast<const T*>(kc), static_cast<const T*>(vc), ldkv, static_cast<const T*>(da), ldda, \
                     static_cast<T*>(out), ldo, len, rows, Lmax, H, scale, n_kv)
  if (Lmax <= 32) RPO_TW(1);
  else if (Lmax <= 64) RPO_TW(2);
  else RPO_TW(3);
#undef RPO_TW
  return rpo_launch_status();
}

}  // namespace

#ifndef RPO_DEVICE_ONLY     // (chain.hip includes this file for the device bodies above)
// 16-bit storage, rows <= 64 prompt queries per class, Lmax <= 96 keys, 16-byte aligned rows: the one-wave kernel above;
// RPO_E_SHAPE otherwise (the caller, attn_text.hip, then runs its VALU kernel).  bwd: `da` = d(attention output), `out` = dq.
int rpo_text_attn_wave(int bwd, const void* q, int64_t ldq, const void* kc, const void* vc, int64_t ldkv, const void* da,
                       int64_t ldda, void* out, int64_t ldo, int dtype, const int32_t* len, int n_cls, int n_kv, int rows,
                       int Lmax, int H, float scale, hipStream_t s) {
  if ((dtype != RPO_BF16 && dtype != RPO_F16) || rows > 64 || Lmax > 96) return RPO_E_SHAPE;
  if (!aligned16(q) || (ldq * 2) % 16 != 0 || (reinterpret_cast<uintptr_t>(out) & 7u) || (ldo * 2) % 8 != 0) return RPO_E_SHAPE;
  if (bwd && (!aligned16(da) || (ldda * 2) % 16 != 0)) return RPO_E_SHAPE;
  if (dtype == RPO_BF16)
    return bwd ? launch_text_wave<bf16_t, true>(q, ldq, kc, vc, ldkv, da, ldda, out, ldo, len, n_cls, n_kv, rows, Lmax, H, scale, s)
               : launch_text_wave<bf16_t, false>(q, ldq, kc, vc, ldkv, da, ldda, out, ldo, len, n_cls, n_kv, rows, Lmax, H, scale, s);
  return bwd ? launch_text_wave<f16_t, true>(q, ldq, kc, vc, ldkv, da, ldda, out, ldo, len, n_cls, n_kv, rows, Lmax, H, scale, s)
             : launch_text_wave<f16_t, false>(q, ldq, kc, vc, ldkv, da, ldda, out, ldo, len, n_cls, n_kv, rows, Lmax, H, scale, s);
}

// LAUNCH<T, NT>(...) by storage type (`dtype`: checked by the caller) and key tiles (`N` <= 224: seven, else nine)
#define RPO_BY_TYPE_NT(LAUNCH, ...)                                                                            \
  do {                                                                                                         \
    if (dtype == RPO_BF16) return N <= 224 ? LAUNCH<bf16_t, 7>(__VA_ARGS__) : LAUNCH<bf16_t, 9>(__VA_ARGS__);  \
    if (dtype == RPO_F16) return N <= 224 ? LAUNCH<f16_t, 7>(__VA_ARGS__) : LAUNCH<f16_t, 9>(__VA_ARGS__);     \
    return N <= 224 ? LAUNCH<float, 7>(__VA_ARGS__) : LAUNCH<float, 9>(__VA_ARGS__);                           \
  } while (0)
// LAUNCH<T>(...) by storage type (the long kernels: the keys in chunks)
#define RPO_BY_TYPE(LAUNCH, ...)                                     \
  do {                                                               \
    if (dtype == RPO_BF16) return LAUNCH<bf16_t>(__VA_ARGS__);       \
    if (dtype == RPO_F16) return LAUNCH<f16_t>(__VA_ARGS__);         \
    return LAUNCH<float>(__VA_ARGS__);                               \
  } while (0)

extern "C" int rpo_attn_readonly_fwd_rows(const void* q, const void* k, const void* v, int64_t ld, void* out,
                                          int64_t ldo, int dtype, int B, int H, int N, int Kp, float scale,
                                          int q_first, void* stream);

extern "C" int rpo_attn_readonly_fwd(const void* q, const void* k, const void* v, int64_t ld, void* out,
                                     int64_t ldo, int dtype, int B, int H, int N, int Kp, float scale,
                                     void* stream) {
  return rpo_attn_readonly_fwd_rows(q, k, v, ld, out, ldo, dtype, B, H, N, Kp, scale, 0, stream);
}

extern "C" int rpo_attn_readonly_fwd_rows(const void* q, const void* k, const void* v, int64_t ld, void* out,
                                          int64_t ldo, int dtype, int B, int H, int N, int Kp, float scale,
                                          int q_first, void* stream) {
  if (!q || !k || !v || !out || B <= 0 || H <= 0 || N <= 0 || Kp < 0 || q_first < 0 || q_first >= N + Kp)
    return RPO_E_BADARG;
  if (N > ATTN_LONG_MAX_N) return RPO_E_SHAPE;
  if (dtype != RPO_F32 && dtype != RPO_BF16 && dtype != RPO_F16) return RPO_E_DTYPE;
  const int esz = dtype == RPO_F32 ? 4 : 2;
  if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !ok_ld(ld, esz) ||
      reinterpret_cast<uintptr_t>(out) % (4 * esz) || (ldo * esz) % (4 * esz)) return RPO_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (N > 288) RPO_BY_TYPE(launch_fwd_long, q, k, v, ld, out, ldo, B, H, N, Kp, scale, q_first, s);   // the keys in chunks
  RPO_BY_TYPE_NT(launch_fwd, q, k, v, ld, out, ldo, B, H, N, Kp, scale, q_first, s);
}

extern "C" int rpo_attn_prompt_fwd(const void* q_rows, int64_t ldq, const void* k, const void* v, int64_t ldkv,
                                   void* out, int64_t ldo, int dtype, int B, int H, int N, int Kp, int sets,
                                   const int32_t* first_image, float scale, void* stream) {
  if (!q_rows || !k || !v || !out || B <= 0 || H <= 0 || N <= 0 || Kp <= 0 || sets <= 0) return RPO_E_BADARG;
  if (N > 288 || (int64_t)sets * Kp > (1 << 24) || (int64_t)sets * Kp * B > INT32_MAX) return RPO_E_SHAPE;
  if (dtype != RPO_F32 && dtype != RPO_BF16 && dtype != RPO_F16) return RPO_E_DTYPE;
  const int esz = dtype == RPO_F32 ? 4 : 2;
  if (!aligned16(q_rows) || !aligned16(k) || !aligned16(v) || !ok_ld(ldq, esz) || !ok_ld(ldkv, esz) ||
      reinterpret_cast<uintptr_t>(out) % (4 * esz) || (ldo * esz) % (4 * esz) ||
      reinterpret_cast<uintptr_t>(first_image) % 4) return RPO_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);
  RPO_BY_TYPE_NT(launch_prompt_fwd, q_rows, ldq, k, v, ldkv, out, ldo, B, H, N, Kp, sets, first_image, scale, s);
}

extern "C" int rpo_attn_prompt_bwd(const void* q_rows, int64_t ldq, const void* k, const void* v, int64_t ldkv,
                                   const void* da, int64_t ldda, void* dq, int64_t lddq, int dtype, int B, int H, int N,
                                   int Kp, int sets, const int32_t* first_image, float scale, void* stream) {
  if (!q_rows || !k || !v || !da || !dq || B <= 0 || H <= 0 || N <= 0 || Kp <= 0 || sets <= 0) return RPO_E_BADARG;
  if (N > 288 || (int64_t)sets * Kp > (1 << 24) || (int64_t)sets * Kp * B > INT32_MAX || (int64_t)B * H > INT32_MAX)
    return RPO_E_SHAPE;
  if (dtype != RPO_F32 && dtype != RPO_BF16 && dtype != RPO_F16) return RPO_E_DTYPE;
  const int esz = dtype == RPO_F32 ? 4 : 2;
  if (!aligned16(q_rows) || !aligned16(k) || !aligned16(v) || !aligned16(da) || !ok_ld(ldq, esz) || !ok_ld(ldkv, esz) ||
      !ok_ld(ldda, esz) || reinterpret_cast<uintptr_t>(dq) % (4 * esz) || (lddq * esz) % (4 * esz) ||
      reinterpret_cast<uintptr_t>(first_image) % 4) return RPO_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);
  RPO_BY_TYPE_NT(launch_prompt_bwd, q_rows, ldq, k, v, ldkv, da, ldda, dq, lddq, B, H, N, Kp, sets, first_image, scale, s);
}

extern "C" int rpo_attn_readonly_bwd(const void* q_rows, int64_t ldq, const void* k, const void* v,
                                     int64_t ldkv, const void* da, int64_t ldda, void* dq, int64_t lddq,
                                     int dtype, int B, int H, int N, int Kp, float scale, void* stream) {
  if (!q_rows || !k || !v || !da || !dq || B <= 0 || H <= 0 || N <= 0 || Kp <= 0) return RPO_E_BADARG;
  if (N > ATTN_LONG_MAX_N || Kp > 128) return RPO_E_SHAPE;
  if (dtype != RPO_F32 && dtype != RPO_BF16 && dtype != RPO_F16) return RPO_E_DTYPE;
  const int esz = dtype == RPO_F32 ? 4 : 2;
  if (!aligned16(q_rows) || !aligned16(k) || !aligned16(v) || !aligned16(da) || !ok_ld(ldq, esz) ||
      !ok_ld(ldkv, esz) || !ok_ld(ldda, esz) || reinterpret_cast<uintptr_t>(dq) % (4 * esz) ||
      (lddq * esz) % (4 * esz)) return RPO_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (N > 288)                                     // the keys in chunks (attn_bwd_long_kernel)
    RPO_BY_TYPE(launch_bwd_long, q_rows, ldq, k, v, ldkv, da, ldda, dq, lddq, B, H, N, Kp, scale, s);
  const AttnBwdProblem a{q_rows, ldq, k, v, ldkv, da, ldda, dq, lddq, B, H, N, Kp, scale, nullptr, 0, nullptr, 0};
  RPO_BY_TYPE_NT(launch_bwd, a, 1, s);             // one workgroup per (image, head) walks the (Kp + 31) / 32 query tiles
}

extern "C" int rpo_attn_readonly_bwd_proj(const void* q_rows, int64_t ldq, const void* k, const void* v, int64_t ldkv,
                                          const void* dx, int64_t lddx, const void* w_out_t, int64_t ldw, void* dq,
                                          int64_t lddq, int dtype, int B, int H, int N, int Kp, float scale,
                                          void* stream) {
  if (!q_rows || !k || !v || !dx || !w_out_t || !dq || B <= 0 || H <= 0 || N <= 0 || Kp <= 0) return RPO_E_BADARG;
  if (dtype != RPO_BF16 && dtype != RPO_F16) return RPO_E_DTYPE;
  const int d = H * 64;
  // Kp > 32: one workgroup per 32-query tile (each stages the keys again); d = 1024: four weight slots per wave
  if (N > 288 || Kp > 64 || (d != 512 && d != 768 && d != 1024)) return RPO_E_SHAPE;
  if (!aligned16(q_rows) || !aligned16(k) || !aligned16(v) || !aligned16(dx) || !aligned16(w_out_t) || !ok_ld(ldq, 2) ||
      !ok_ld(ldkv, 2) || !ok_ld(lddx, 2) || !ok_ld(ldw, 2) || reinterpret_cast<uintptr_t>(dq) % 8 || (lddq * 2) % 8)
    return RPO_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const AttnBwdProblem a{q_rows, ldq, k, v, ldkv, dx, lddx, dq, lddq, B, H, N, Kp, scale, w_out_t, ldw, nullptr, 0};
  if (dtype == RPO_BF16) return dispatch_bwd_proj<bf16_t>(d / 256, N > 224, a, s);
  return dispatch_bwd_proj<f16_t>(d / 256, N > 224, a, s);
}

// rpo_attn_readonly_bwd_proj for one or two problems in ONE launch, each with optional per-group key counts
// (include/rpo_amd.h: rpo_attn_bwd_args).  a1 == NULL: one problem.
#ifdef RPO_EXPERIMENTAL   // measured-slower experiment: include/rpo_amd_experimental.h
extern "C" int rpo_attn_bwd_proj_pair(const rpo_attn_bwd_args* a0, const rpo_attn_bwd_args* a1, int dtype, void* stream) {
  if (a0 == nullptr) return RPO_E_BADARG;
  if (dtype != RPO_BF16 && dtype != RPO_F16) return RPO_E_DTYPE;
  if (int rc = bwd_proj_check(*a0)) return rc;
  if (a1 != nullptr) if (int rc = bwd_proj_check(*a1)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dtype == RPO_BF16) return dispatch_bwd_proj_args<bf16_t>(a0, a1, s);
  return dispatch_bwd_proj_args<f16_t>(a0, a1, s);
}
#endif  // RPO_EXPERIMENTAL
#endif  // RPO_DEVICE_ONLY
