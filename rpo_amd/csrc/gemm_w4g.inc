// gemm_w4g.inc -- included by gemm.hip inside its anonymous namespace, after gemm_w4.inc (uses GemmParams, make_srd,
// ln_finish, quick_gelu).
//
// ---- one-wave-per-SIMD 224x384 kernel: one ROUND for c_fc ----------------------------------------------------------
// c_fc at B = 32 (7072 x 3072 x 768) is 336 tiles of 256x256: 1.31 rounds of the 256 CUs, so the 256x256 kernel of
// gemm_w4.inc pays two full rounds (54 us, no better than the 8-wave 128x128 tiles).  7072 = 32 x 221 and
// 3072 = 8 x 384: tiles of 221 rows (224 loaded: 7 x 32) x 384 columns cover it with exactly 32 x 8 = 256 workgroups,
// one per CU, one round, 1.4 % padding.  Four waves side by side along N, each 224 x 96 = 7 x 3 MFMA tiles:
//   * 21 accumulators (336 registers: 256 AGPR + 80 VGPR) + two fragment sets of 10 (80 VGPR): fits the 512-entry file
//     of a wave alone on its SIMD;
//   * per 16-deep k-step 10 fragment reads feed 21 MFMAs (0.48 reads per MFMA, as the 256x256 kernel), 19 DMA pieces
//     per 64-deep k-tile and wave = one per 4.4 MFMAs;
//   * LDS: 2 slots x (224 + 384) rows x 128 B = 152 KiB.
// k-loop: generated (tools/gen_gemm_w4.py -> gemm_w4g_asm.inc), same structure and hazard arguments as gemm_w4.inc:
// p0 / p1 fetch the W pieces of tile t+1, p2 front-loads its reads, lgkmcnt(0) + vmcnt(0) + barrier, p3 reads tile
// t+1 and fetches the A pieces of tile t+2 into the slot tile t just left.
//
// Epilogue: per WAVE, no workgroup barrier.  A wave converts 32 rows x 96 columns at a time (LayerNorm fold / bias /
// QuickGELU in the fragment layout), parks them as 16-bit in its private 6.5 KiB of LDS and walks them back row-major
// (16-B stores of 192-B row segments).  LDS operations of one wave execute in order, so write -> read -> next write
// needs no wait beyond the data dependency; the stores are fire-and-forget, so the store drain of one 32-row block
// overlaps the VALU work (two quarter-rate transcendentals per element) of the next -- with one wave per SIMD nothing
// else would.
#include "gemm_w4g_asm.inc"

// Two geometries of the same kernel (k-loops: W4G_LOOP_7X3 / W4G_LOOP_9X2 of gemm_w4g_asm.inc):
//   7 x 3: tile 224 x 384, a wave 224 x 96 -- ViT-B/16: 197 + K <= 224 rows per image, 3072 = 8 x 384
//   9 x 2: tile 288 x 256, a wave 288 x 64 -- ViT-L/14: 257 + K <= 288 rows per image, 4096 = 16 x 256 (16 images: 256 tiles)
template <int TM_, int TN_>
struct CfgW4GT {
  static constexpr int TM = TM_, TN = TN_, WN = TN_ * 32;           // WN: columns of one wave
  static constexpr int BM = TM_ * 32, BN = 4 * WN, BK = 64, THREADS = 256;
  static constexpr int A_BYTES = BM * 128, SLOT_BYTES = (BM + BN) * 128;
  static constexpr int STATS_OFF = 2 * SLOT_BYTES;                  // (mu, rstd) per row of the LayerNorm fold
  static constexpr int SMEM = STATS_OFF + BM * 8;
  static constexpr int STG_ROW = WN * 2 + 16, STG_BYTES = 32 * STG_ROW;   // per-wave staging block
};
using CfgW4G = CfgW4GT<7, 3>;
using CfgW4GL = CfgW4GT<9, 2>;

// (the body as a device function: gemm_mlp.inc runs it and the 224x96 kernel's body back to back in ONE launch)
template <typename TOut, int EPI, typename CF>
__device__ __forceinline__ void gemm_w4g_body(const GemmParams p, const int rows0, const int rows1,
                                              const int seg1_base, const int tiles_n, char* const smem) {
  constexpr bool IS_LN = EPI == RPO_EPI_LN_BIAS || EPI == RPO_EPI_LN_BIAS_QGELU;
  constexpr bool IS_QG = EPI == RPO_EPI_BIAS_QGELU || EPI == RPO_EPI_LN_BIAS_QGELU;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);       // = column block of 96
  const int half = lane >> 5, l31 = lane & 31;
  RPO_STAMP(0); RPO_STAMP_RT(62);
  // Workgroup -> tile.  Block b runs on XCD b % 8; an XCD takes whole row units (all column tiles of a unit), the same
  // units it handled in the out-proj kernel (gemm_w4k.inc) that has just written this kernel's A rows and the same it
  // will handle in c_proj, which reads this kernel's output: producer and consumer of a row meet in one L2.  Inside a
  // training step this beats "one weight panel per XCD" by 1 % of the step, although in a warm loop of this kernel alone
  // the two orders measure the same.
  int tile_m, tile_n;
  {
    const int nwg = gridDim.x, bid = blockIdx.x;
    const int wg = xcd_run(bid, nwg);
    tile_m = wg / tiles_n;
    tile_n = wg - tile_m * tiles_n;
  }
  const int n0 = tile_n * CF::BN;
  const int nk = p.K / CF::BK;                                      // the launcher guarantees nk >= 2
  // Rows of the tile: rows0 rows of segment 0 ([0, seg1_base)) followed by rows1 rows of segment 1 ([seg1_base, M)) --
  // in the image tower one image's frozen rows and its prompt rows, so that every workgroup holds the same number of
  // back-propagated rows.  (With contiguous tiles the 768 prompt rows at the end of the stream fall into 3.5 of the 32
  // row tiles, whose workgroups then store three times the bytes of the others: a CU retires about 20 B of stores per
  // clock, and c_fc ended 11 us later than without the saved pre-activations.)  rows1 = 0: plain contiguous tiles.
  const int seg0_end = rows1 > 0 ? seg1_base : p.M;
  auto row_raw = [&](int r) -> int {                                // tile row -> row of A / C, before the bounds
    return r < rows0 ? tile_m * rows0 + r : seg1_base + tile_m * rows1 + (r - rows0);
  };
  auto row_of = [&](int r) -> int {                                 // ... or -1 for rows the tile does not own
    const int m = row_raw(r);
    return r < rows0 ? (m < seg0_end ? m : -1) : (r < rows0 + rows1 && m < p.M ? m : -1);
  };

  // DMA: one instruction = 8 rows x 128 B; wave w owns pieces 4 * i + w: rows 32 * i + 8 * w + (lane >> 3)
  const int drow = 8 * wave + (lane >> 3);
  const int dchunk = (lane & 7) ^ ((drow >> 1) & 7);
  uint32_t offa[CF::TM];
#pragma unroll
  for (int i = 0; i < CF::TM; ++i) {
    const int m = row_of(32 * i + drow);                            // rows outside the tile: out of range -> zeros
    offa[i] = m < 0 ? 0x80000000u : (uint32_t)m * (uint32_t)(p.lda * 2) + dchunk * 16;
  }
  const uint32_t offw = (uint32_t)(n0 + drow) * (uint32_t)(p.ldw * 2) + dchunk * 16;
  const rpo_srd_t srda = make_srd(p.A, (uint32_t)p.M * (uint32_t)(p.lda * 2));
  const rpo_srd_t srdw = make_srd(p.W, (uint32_t)p.N * (uint32_t)(p.ldw * 2));
  const uint32_t rsw = 32u * (uint32_t)(p.ldw * 2);
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  const uint32_t lds_w = lds0 + wave * 1024;
  if (lds0 & 127u) __builtin_trap();

  f32x16_t acc[CF::TN][CF::TM];
#pragma unroll
  for (int a = 0; a < CF::TN; ++a)
#pragma unroll
    for (int b = 0; b < CF::TM; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.0f;

  // fragment read addresses of k-step 0: A rows tm*32 + l31 (every wave reads all of them), W rows wave*96 + tn*32 + l31
  const int sw = (l31 >> 1) & 7;
  const uint32_t ax0 = lds0 + l31 * 128 + ((half ^ sw) << 4);
  const uint32_t aw0 = lds0 + CF::A_BYTES + (wave * CF::WN + l31) * 128 + ((half ^ sw) << 4);
  const uint32_t nloop = (uint32_t)(nk - 2);

  // LayerNorm fold: partial row statistics requested before the loop, reduced after it (one row per thread, and a second
  // one for the first BM - 256 threads of the 288-row tile)
  constexpr int RPT = (CF::BM + 255) / 256;
  float2 lnp[RPT][16];
  if constexpr (IS_LN) {
    const int G = p.K / p.ln_group;
#pragma unroll
    for (int rr = 0; rr < RPT; ++rr) {
      const float2* ps = reinterpret_cast<const float2*>(p.ln_stats) +
                         (int64_t)max(row_of(min(tid + 256 * rr, CF::BM - 1)), 0) * G;
#pragma unroll
      for (int g = 0; g < 16; ++g) lnp[rr][g] = ps[min(g, G - 1)];
    }
  }
  // next kernel's weights -> memory-side cache (GemmParams::pf_ptr).  Not in the LN_BIAS instance of this geometry: one
  // more VGPR live across the loop tips hipcc's allocation of its epilogue into 183 spills (the in-proj shapes that hint
  // run on gemm_w4_kernel)
  uint32_t pf_touch = 0;
  if constexpr (!(EPI == RPO_EPI_LN_BIAS && CF::TM == 7)) pf_touch = prefetch_touch(p);
  RPO_STAMP(2);
  W4G_KLOOP(CF, (__is_same(TOut, f16_t)));                         // gemm_w4g_asm.inc: loop and operand list of this geometry
  RPO_STAMP(60);
  asm volatile("" :: "v"(pf_touch));

  // ---- epilogue (per wave) -----------------------------------------------------------------------------------------
  float2* row_stats = reinterpret_cast<float2*>(smem + CF::STATS_OFF);
  if constexpr (IS_LN) {
#pragma unroll
    for (int rr = 0; rr < RPT; ++rr)
      if (tid + 256 * rr < CF::BM) {
        const int G = p.K / p.ln_group;
        float mu = 0.f, m2 = 0.f, sq = 0.f;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
          const float mg = g < G ? lnp[rr][g].x : 0.f;
          mu += mg; m2 += g < G ? lnp[rr][g].y : 0.f; sq = fmaf(mg, mg, sq);
        }
        row_stats[tid + 256 * rr] = ln_finish(mu, m2, sq, G, p.K, p.ln_eps);
      }
    __syncthreads();
  }
  // staging: the slot the LAST tile did not use (dead since the last barrier of the loop; the other slot may still be
  // read by slower waves)
  char* st = smem + (nk & 1) * CF::SLOT_BYTES + wave * CF::STG_BYTES;
  const int nw = n0 + wave * CF::WN;                                // first column of this wave
  const int r_last = min(rows0 + rows1, CF::BM) - 1;                // last row of the tile (rows ascend with r)
  const bool tile_saves_u = IS_QG && p.aux != nullptr && row_raw(r_last) >= p.aux_row0;   // uniform, conservative
  uint16_t* cbase = reinterpret_cast<uint16_t*>(p.C);
  // bias (and column sums) of this lane's 12 column quads are fetched ONCE, before the first store: a global load
  // inside the block loop makes hipcc wait vmcnt(0) for it -- on gfx950 stores count in vmcnt and return out of order
  // with loads -- i.e. drain every store of the previous block before the next block's arithmetic; reading them back
  // from LDS per quad instead put an LDS round trip (ds_read -> lgkmcnt(0)) in front of every quad.  The fragment
  // registers of the k-loop are dead here, so the 48 (96) VGPRs are free.
  float4 b4r[CF::TN][4], s4r[CF::TN][4];
#pragma unroll
  for (int tn = 0; tn < CF::TN; ++tn)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int n = min(nw + tn * 32 + 8 * g + 4 * half, p.N - 4);
      b4r[tn][g] = *reinterpret_cast<const float4*>(p.bias + n);
      if constexpr (IS_LN) s4r[tn][g] = *reinterpret_cast<const float4*>(p.ln_colsum + n);
    }
  // v = LayerNorm fold / bias of one accumulator quad
  auto pre_act = [&](float a0, float a1, float a2, float a3, float2 stt, int tn, int g) -> float4 {
    const float4 b4 = b4r[tn][g];
    if constexpr (IS_LN) {
      const float4 s4 = s4r[tn][g];
      return make_float4(fmaf(stt.y, a0 - stt.x * s4.x, b4.x), fmaf(stt.y, a1 - stt.x * s4.y, b4.y),
                         fmaf(stt.y, a2 - stt.x * s4.z, b4.z), fmaf(stt.y, a3 - stt.x * s4.w, b4.w));
    } else {
      return make_float4(a0 + b4.x, a1 + b4.y, a2 + b4.z, a3 + b4.w);
    }
  };
  // Pre-activations of the back-propagated rows: only the few tiles that hold such rows run this pass, and it is kept
  // OUT of the block loop below -- a per-quad `if` there splits the loop into 4-element basic blocks, which leaves the
  // mul -> exp -> add -> rcp -> mul chains of QuickGELU without independent work to hide their latency.
  // 16-bit modes with the derivative saved in the act dtype (aux_mode 1): formed in the block loop below, from the
  // sigmoid the activation computes anyway (no second pre_act / v_exp / v_rcp pass, no fp32 LDS round trip: the separate
  // pass cost 7-8 k of the kernel's 70 k cycles, profiles/r03_gemm_timeline.txt "+ saved QuickGELU operand" rows)
#ifdef RPO_W4G_SEPARATE_DU        // ablation build: the separate pass for every form of the saved operand
  const bool fuse_du = false;
#else
  const bool fuse_du = IS_QG && tile_saves_u && p.aux_mode != 0 && (p.ldaux & 7) == 0;
#endif
  if constexpr (IS_QG) {
    if (tile_saves_u && !fuse_du) {
      // fp32, through the same kind of per-wave LDS block (32 rows x 96 floats), so that the global stores are whole
      // 384-B row segments (straight from the fragment layout a store instruction would touch 32 rows x 32 B)
      constexpr int FROW = CF::WN * 4 + 16, FCH = CF::WN / 4;      // fp32 staging row, 16-B chunks per row
      char* stf = smem + (nk & 1) * CF::SLOT_BYTES + 4 * CF::STG_BYTES + wave * (32 * FROW);
#pragma unroll
      for (int tm = 0; tm < CF::TM; ++tm) {
        if (tm * 32 > r_last || row_raw(min(tm * 32 + 31, r_last)) < p.aux_row0) continue;   // uniform: no saved row
        float2 stt = make_float2(0.f, 1.f);
        if constexpr (IS_LN) stt = row_stats[tm * 32 + l31];
#pragma unroll
        for (int tn = 0; tn < CF::TN; ++tn)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int col = tn * 32 + 8 * g + 4 * half;
            *reinterpret_cast<float4*>(stf + l31 * FROW + col * 4) =
                pre_act(acc[tn][tm][4 * g], acc[tn][tm][4 * g + 1], acc[tn][tm][4 * g + 2], acc[tn][tm][4 * g + 3], stt, tn, g);
          }
#pragma unroll
        for (int it = 0; it < FCH / 2; ++it) {
          const int idx = it * 64 + lane;
          const int row = idx / FCH, ch = idx - row * FCH;
          const float4 v = *reinterpret_cast<const float4*>(stf + row * FROW + ch * 16);
          const int m = row_of(tm * 32 + row);
          if (m >= p.aux_row0 && nw + ch * 4 < p.N)      // fp32 u, or d quickgelu / du in the act dtype (gemm.hip: aux_store4)
            aux_store4<TOut>(p, (int64_t)(m - p.aux_row0) * p.ldaux + nw + ch * 4, v);
        }
      }
    }
  }
  // Store addressing, once per lane instead of per store (the epilogue is VALU-bound; per store the generic form --
  // tile row -> matrix row with its bounds, 64-bit multiply by ldc -- was ~20 VALU instructions, two of them
  // quarter-rate): the block of 32 rows x WN columns is written as CH / 2 stores per lane, store `it` of a lane always
  // to the same (row, 16-B chunk) of the block.  Address = uniform base of the block (SGPRs) + a 32-bit lane offset;
  // rows of segment 1 lie `dseg` bytes further (the launcher admits the kernel only if C spans < 2 GB).
  constexpr int CH = CF::WN / 8;
  int srow[CH / 2];
  uint32_t soff[CH / 2];
#pragma unroll
  for (int it = 0; it < CH / 2; ++it) {
    const int idx = it * 64 + lane;
    const int row = idx / CH, ch = idx - row * CH;
    srow[it] = nw + ch * 8 < p.N ? row : (1 << 24);
    soff[it] = (uint32_t)(row * (int)p.ldc + ch * 8) * 2u;
  }
  const int nv0 = max(0, min(rows0, seg0_end - tile_m * rows0));                        // valid rows of segment 0 ...
  const int lim1 = rows0 + (rows1 > 0 ? max(0, min(rows1, p.M - (seg1_base + tile_m * rows1))) : 0);   // ... and of 1
  char* const cb0 = reinterpret_cast<char*>(cbase) + ((int64_t)tile_m * rows0 * p.ldc + nw) * 2;
  const uint32_t dseg = (uint32_t)(((int64_t)seg1_base + (int64_t)tile_m * rows1 - rows0 - (int64_t)tile_m * rows0) * p.ldc * 2);
  char* const st_du = smem + (nk & 1) * CF::SLOT_BYTES + (4 + wave) * CF::STG_BYTES;   // second per-wave block: d quickgelu / du
#pragma unroll
  for (int tm = 0; tm < CF::TM; ++tm) {
    float2 stt = make_float2(0.f, 1.f);
    if constexpr (IS_LN) stt = row_stats[tm * 32 + l31];
    bool with_du = false;                                           // uniform: this block holds back-propagated rows
    if constexpr (IS_QG) with_du = fuse_du && tm * 32 <= r_last && row_raw(min(tm * 32 + 31, r_last)) >= p.aux_row0;
    if (with_du) {
      if constexpr (IS_QG) {
#pragma unroll
        for (int tn = 0; tn < CF::TN; ++tn)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int col = tn * 32 + 8 * g + 4 * half;
            const float4 u = pre_act(acc[tn][tm][4 * g], acc[tn][tm][4 * g + 1], acc[tn][tm][4 * g + 2], acc[tn][tm][4 * g + 3], stt, tn, g);
            float4 v, d;
            quick_gelu4_du(u, v, d);
            *reinterpret_cast<uint2*>(st + l31 * CF::STG_ROW + col * 2) = make_uint2(pack2<TOut>(v.x, v.y), pack2<TOut>(v.z, v.w));
            *reinterpret_cast<uint2*>(st_du + l31 * CF::STG_ROW + col * 2) = make_uint2(pack2<TOut>(d.x, d.y), pack2<TOut>(d.z, d.w));
          }
      }
    } else {
#pragma unroll
      for (int tn = 0; tn < CF::TN; ++tn)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int col = tn * 32 + 8 * g + 4 * half;                 // within the wave's 96 columns
          float4 v = pre_act(acc[tn][tm][4 * g], acc[tn][tm][4 * g + 1], acc[tn][tm][4 * g + 2], acc[tn][tm][4 * g + 3], stt, tn, g);
          if constexpr (IS_QG) { v = quick_gelu4(v); }
          *reinterpret_cast<uint2*>(st + l31 * CF::STG_ROW + col * 2) = make_uint2(pack2<TOut>(v.x, v.y), pack2<TOut>(v.z, v.w));
        }
    }
    // row-major: 32 rows x CH chunks of 16 B
    char* const cb = cb0 + (int64_t)(tm * 32) * p.ldc * 2;          // uniform
#pragma unroll
    for (int it = 0; it < CH / 2; ++it) {
      const int idx = it * 64 + lane;
      const int row = idx / CH, ch = idx - row * CH;
      const uint4 v = *reinterpret_cast<const uint4*>(st + row * CF::STG_ROW + ch * 16);
#ifdef RPO_W4G_NOSTORE            // ablation build: keep the LDS round trip alive, skip the global store
      asm volatile("" :: "v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w));
#else
      const int r = tm * 32 + srow[it];
      const bool s0 = r < rows0;
      if (r < (s0 ? nv0 : lim1)) store_out16(reinterpret_cast<uint4*>(cb + (size_t)(soff[it] + (s0 ? 0u : dseg))), v);
#endif
    }
    if (with_du) {
#pragma unroll
      for (int it = 0; it < CH / 2; ++it) {
        const int idx = it * 64 + lane;
        const int row = idx / CH, ch = idx - row * CH;
        const uint4 v = *reinterpret_cast<const uint4*>(st_du + row * CF::STG_ROW + ch * 16);
        const int m = row_of(tm * 32 + row);
        if (m >= p.aux_row0 && nw + ch * 8 < p.N)
          store_out16(reinterpret_cast<uint4*>(reinterpret_cast<TOut*>(p.aux) + (int64_t)(m - p.aux_row0) * p.ldaux + nw + ch * 8), v);
      }
    }
  }
#ifdef RPO_TIMELINE
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
  RPO_STAMP(61); RPO_STAMP_RT(63);
}

template <typename TOut, int EPI, typename CF>
__global__ __launch_bounds__(256, 1) void gemm_w4g_kernel(const GemmParams p, const int rows0, const int rows1,
                                                          const int seg1_base, const int tiles_n) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  gemm_w4g_body<TOut, EPI, CF>(p, rows0, rows1, seg1_base, tiles_n, smem);
}

// Tiling of the 224x384 kernel for an [M, N] output, or false if it does not apply: N a multiple of 384, the tiles fit
// ONE round of the 256 CUs and fill most of it.  With the caller's row-unit hint (rpo_gemm_args.seg_*) one tile = one
// unit; otherwise contiguous tiles of equal height.
template <typename CF>
static inline bool w4g_plan_t(const GemmParams& p, W4RowsPlan* q) {
  if (p.N % CF::BN != 0 || (int64_t)p.M * p.ldc * 2 >= (int64_t(1) << 31)) return false;   // 32-bit store offsets
  if (w4_unit_plan<CF>(p, q)) return true;
  const int tn = p.N / CF::BN, tm = (p.M + CF::BM - 1) / CF::BM;
  if (!w4_rounds_ok(tm * tn)) return false;
  *q = W4RowsPlan{(p.M + tm - 1) / tm, 0, p.M, tm, tn, false, CF::TM};
  return true;
}
// 0: no geometry applies; 1: 224 x 384 tiles; 2: 288 x 256 tiles
static inline int w4g_plan(const GemmParams& p, W4RowsPlan* q) {
  if (w4g_plan_t<CfgW4G>(p, q)) return 1;
  if (w4g_plan_t<CfgW4GL>(p, q)) return 2;
  return 0;
}

template <typename TOut, int EPI>
int launch_w4g(const GemmParams& p, hipStream_t s) {
  W4RowsPlan q;
  switch (w4g_plan(p, &q)) {
    case 1: return launch_w4_rows<gemm_w4g_kernel<TOut, EPI, CfgW4G>, CfgW4G>(p, q, s);
    case 2: return launch_w4_rows<gemm_w4g_kernel<TOut, EPI, CfgW4GL>, CfgW4GL>(p, q, s);
    default: return RPO_E_SHAPE;
  }
}
