// gemm_w4k.inc -- included by gemm.hip inside its anonymous namespace, after gemm_w4g.inc (uses GemmParams, make_srd).
//
// ---- 224x96 tiles, the four waves split k: the N = 768 GEMMs (out-proj, c_proj) in ONE round ------------------------
// out-proj / c_proj at B = 32 (7072 x 768 x {768, 3072}) are bound by the LDS-DMA stream, not by MFMA: their 64x128
// tiles move M N K 2 (1/64 + 1/128) = 782 MB through the DMA path for c_proj, and 782 MB / 55.7 us = 14 TB/s is what
// tools/ubench_dma.hip measures as the chip-wide DMA rate (profiles/r02_ubench_dma.txt).  Bigger tiles are the only
// lever, but 256x256 (84 tiles) or 224x384 (64) leave most CUs idle at N = 768.  One image = 221 rows and
// 768 = 8 x 96: tiles of one row unit x 96 columns are exactly 32 x 8 = 256 workgroups, one per CU, and move
// M N K 2 (1/224 + 1/96) = 491 MB.  A 224x96 tile is ONE wave's worth of accumulators in the 224x384 kernel
// (7 x 3 MFMA tiles, 336 registers), so here every wave holds the whole tile and the waves split the CONTRACTION:
// wave w multiplies k-step w (16 of the 64 k's) of every k-tile.  Nothing staged in LDS is read twice -- LDS is only
// the landing zone of the DMA -- so per wave and k-tile the loop is 10 DMA pieces, 10 fragment reads, 21 MFMAs
// (tools/gen_gemm_w4.py -> gemm_w4k_asm.inc).  The four partial tiles are summed in a fixed order by the epilogue
// (through LDS, 32 rows at a time), which then does what the BIAS_RESID epilogue of the other kernels does: bias +
// residual -> fp32 C, the 16-bit copy (out2) and the partial LayerNorm statistics of the row -- over the tile's 96
// columns (rpo_gemm_args.ln_group = 96).
//
// Results: deterministic; NOT bit-identical to the other tile shapes (four-way split of the k sum).
#include "gemm_w4k_asm.inc"

// Three geometries (k-loops: W4K_LOOP_7X3 / W4K_LOOP_9X2 / W4K_LOOP_8X3 of gemm_w4k_asm.inc):
//   7 x 3, ring of 4: tile 224 x 96 -- ViT-B/16: 197 + K <= 224 rows per image, 768 = 8 x 96, statistics over 96 columns
//   8 x 3, ring of 3: tile 256 x 96 -- ViT-B/16 with 225 .. 256 rows per image (K = 48: 245); 384 accumulator registers
//                     (256 AGPR + 128 VGPR), its unrolled body entered like the 9 x 2 one
//   9 x 2, ring of 3: tile 288 x 64 -- ViT-L/14: 257 + K <= 288 rows per image, 1024 = 16 x 64 (16 images: 256 tiles),
//                     statistics over 64 columns; its unrolled body is 6 iterations, entered at position `entry`
template <int TM_, int TN_, int RING_>
struct CfgW4KT {
  static constexpr int TM = TM_, TN = TN_, RING = RING_, UNROLL = RING_ % 2 ? 2 * RING_ : RING_;
  static constexpr int BM = TM_ * 32, BN = TN_ * 32, BK = 64, THREADS = 256;
  static constexpr int A_BYTES = BM * 128, SLOT_BYTES = (BM + BN) * 128;
  static constexpr int SMEM = RING * SLOT_BYTES;                    // 7 x 3: 163840, the whole LDS of a CU
  static constexpr int FROW = BN * 4 + 16;                          // fp32 staging row of the reduction
  static constexpr int PART_BYTES = 32 * FROW;                      // one wave's 32-row partial block
};
using CfgW4K = CfgW4KT<7, 3, 4>;
using CfgW4KL = CfgW4KT<9, 2, 3>;
using CfgW4K8 = CfgW4KT<8, 3, 3>;    // round 4: 225 .. 256 rows per unit (ViT-B/16 at K = 48: 245), 768 = 8 x 96

// sum over the 8 lanes (lane & ~7) .. (lane | 7): two quad permutes and a half-row mirror, one VALU each
__device__ __forceinline__ float row8_sum(float v) {
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xf, 0xf, false));    // quad_perm [1,0,3,2]
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xf, 0xf, false));    // quad_perm [2,3,0,1]
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xf, 0xf, false));   // row_half_mirror
  return v;
}

template <typename TAct, typename CF>
__device__ __forceinline__ void gemm_w4k_body(const GemmParams p, const int rows0, const int rows1,
                                              const int seg1_base, const int tiles_n, char* const smem) {
  constexpr int NJ = CF::TN;                                        // 32-column thirds / halves of the tile
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);       // = k-step of every k-tile
  const int half = lane >> 5, l31 = lane & 31;
  RPO_STAMP(0); RPO_STAMP_RT(62);
  // Workgroup -> tile: block b runs on XCD b % 8; an XCD takes whole row units (all column tiles of a unit read the
  // same A panel, which then comes out of that XCD's L2 after the first fetch)
  int tile_m, tile_n;
  {
    const int nwg = gridDim.x, bid = blockIdx.x;
    const int wg = xcd_run(bid, nwg);
    tile_m = wg / tiles_n;
    tile_n = wg - tile_m * tiles_n;
  }
  const int n0 = tile_n * CF::BN;
  const int nk = p.K / CF::BK;                                      // the launcher guarantees an admitted nk (w4k_plan_t)
  const int seg0_end = rows1 > 0 ? seg1_base : p.M;
  auto row_of = [&](int r) -> int {                                 // tile row -> row of A / C, or -1 (gemm_w4g.inc)
    const int m = r < rows0 ? tile_m * rows0 + r : seg1_base + tile_m * rows1 + (r - rows0);
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

  // fragment read addresses in slot 0: k-step `wave` = 16-B chunks 2 * wave + half of the (swizzled) 128-B row
  const int sw = (l31 >> 1) & 7;
  const uint32_t ax0 = lds0 + l31 * 128 + (((2 * wave + half) ^ sw) << 4);
  const uint32_t aw0 = ax0 + CF::A_BYTES;
  // nk - RING iterations fetch; the unrolled body is entered at `entry` so that they end on a body boundary
  const uint32_t entry = (uint32_t)((CF::UNROLL - (nk - CF::RING) % CF::UNROLL) % CF::UNROLL);
  const uint32_t nloop = (uint32_t)((nk - CF::RING + (int)entry) / CF::UNROLL);
  const uint32_t pf_touch = prefetch_touch(p);   // next kernel's weights -> memory-side cache (GemmParams::pf_ptr)
  // EXPERIMENT (round 4, off: -DRPO_W4K_RESID_TOUCH): touch the residual tile of the epilogue (86 KB per workgroup, 22 MB
  // per launch, written a layer ago) here, one dword per 128-B line, so that its fetch runs under the k-loop instead of in
  // front of the epilogue's own store burst.  Thread t takes tile row t; all touches of a thread land in ONE register
  // (in-order returns; the value is never used), requested before the loop's first DMA like the hint above.  Measured
  // same-box, three alternating pairs: step 3.070 ms with the touch against 3.024 ms without (+1.5 %; in-step c_proj
  // 40.8 vs 38.9 us, out-proj 22.8 vs 21.2): the k-loop's DMA stream is what the early fetch competes with, and the
  // XCD's L2 (A panel + W + 2.7 MB of residual > 4 MB) does not keep the lines until the epilogue.
  uint32_t rs_touch = 0;
#ifdef RPO_W4K_RESID_TOUCH
  {
    // branch-free (a copy of rs_touch on a control-flow edge would read it before the loads have landed): four addresses
    // per tile row -- hi / lo halves: first and last dword of the two BN*2-byte segments; fp32: of the BN*4-byte segment
    // and its 128-byte steps -- selected, then ONE asm statement that defines rs_touch
    constexpr int RPT = (CF::BM + 255) / 256;
    const bool hl = p.resid_hi != nullptr;
    const char* ta[RPT][4];
#pragma unroll
    for (int rr = 0; rr < RPT; ++rr) {
      const int m = max(row_of(min(tid + 256 * rr, CF::BM - 1)), 0);
      const char* h = hl ? p.resid_hi + ((int64_t)m * p.ldr16 + n0) * 2
                         : reinterpret_cast<const char*>((p.resid != nullptr ? p.resid : reinterpret_cast<const float*>(p.A)) + (p.resid != nullptr ? (int64_t)m * p.ldr + n0 : 0));
      const char* l = hl ? (p.resid_lo != nullptr ? p.resid_lo + ((int64_t)m * p.ldr16 + n0) * 2 : h) : h + 128;
      const int last = hl ? CF::BN * 2 - 4 : (p.resid != nullptr ? CF::BN * 4 - 4 : 0);
      ta[rr][0] = h; ta[rr][1] = h + last; ta[rr][2] = l; ta[rr][3] = hl ? l + last : (p.resid != nullptr ? h + (CF::BN * 4 > 256 ? 256 : 128) : h);
    }
    if constexpr (RPT == 1)
      asm volatile("global_load_dword %0, %1, off\n\tglobal_load_dword %0, %2, off\n\t"
                   "global_load_dword %0, %3, off\n\tglobal_load_dword %0, %4, off"
                   : "=&v"(rs_touch) : "v"(ta[0][0]), "v"(ta[0][1]), "v"(ta[0][2]), "v"(ta[0][3]) : "memory");
    else
      asm volatile("global_load_dword %0, %1, off\n\tglobal_load_dword %0, %2, off\n\t"
                   "global_load_dword %0, %3, off\n\tglobal_load_dword %0, %4, off\n\t"
                   "global_load_dword %0, %5, off\n\tglobal_load_dword %0, %6, off\n\t"
                   "global_load_dword %0, %7, off\n\tglobal_load_dword %0, %8, off"
                   : "=&v"(rs_touch) : "v"(ta[0][0]), "v"(ta[0][1]), "v"(ta[0][2]), "v"(ta[0][3]),
                     "v"(ta[RPT - 1][0]), "v"(ta[RPT - 1][1]), "v"(ta[RPT - 1][2]), "v"(ta[RPT - 1][3]) : "memory");
  }
#endif
  RPO_STAMP(2);
  W4K_KLOOP(CF, (__is_same(TAct, f16_t)));                         // gemm_w4k_asm.inc: loop and operand list of this geometry
  RPO_STAMP(60);
  asm volatile("" :: "v"(pf_touch), "v"(rs_touch));

  // ---- epilogue: sum the four partial tiles, bias + residual, C / out2 / row statistics ------------------------------
  // 32 rows at a time: every wave parks its 32 x 96 partial block (fragment layout -> row-major fp32), barrier, then
  // wave w finishes rows 8w .. 8w+7 of the block: lane = (row, 16-B column chunk c8 of each 32-column third), i.e.
  // 128-B row segments per 8 lanes.  Two LDS buffers, one barrier per block.
  const int row8 = lane >> 3, c8 = lane & 7;
  // The residual of all 56 rows this wave finishes is requested NOW, in one batch: inside a step it comes from HBM
  // (written a layer ago), and every workgroup of this one-round kernel reaches its epilogue at the same moment, so a
  // load -> use per 32-row block exposed one HBM round trip per block (7 in a row: +5 us against a warm loop).  The
  // fragment registers of the k-loop are dead, so the 84 VGPRs are there.
  // (8 x 3 geometry: 384 accumulator registers leave room for half of it; the second half is requested once the first
  //  accumulator blocks have been parked: RS_FIRST)
  constexpr int RS_FIRST = CF::TM == 8 ? 4 : CF::TM;
  float4 rs[CF::TM][NJ];
  int mrow[CF::TM];
  const bool hilo_in = p.resid_hi != nullptr;                       // (uniform)
  auto two16 = [](uint32_t w) { return make_float2(unpack1<TAct>((uint16_t)(w & 0xffffu)), unpack1<TAct>((uint16_t)(w >> 16))); };
  auto load_resid = [&](const int tm) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      if (hilo_in) {     // residual stream as 16-bit hi / lo halves (rpo_gemm_args.resid_hi): raw bits now, decoded at use
        const int64_t off = ((int64_t)max(mrow[tm], 0) * p.ldr16 + n0 + 32 * j + 4 * c8) * 2;
        const uint2 h2 = *reinterpret_cast<const uint2*>(p.resid_hi + off);
        const uint2 l2 = p.resid_lo != nullptr ? *reinterpret_cast<const uint2*>(p.resid_lo + off) : make_uint2(0u, 0u);   // hi only: a 16-bit stream
        rs[tm][j] = make_float4(__uint_as_float(h2.x), __uint_as_float(h2.y), __uint_as_float(l2.x), __uint_as_float(l2.y));
      } else {
        rs[tm][j] = *reinterpret_cast<const float4*>(p.resid + (int64_t)max(mrow[tm], 0) * p.ldr + n0 + 32 * j + 4 * c8);
      }
    }
  };
  if constexpr (RS_FIRST == CF::TM) {
    // (written out, not through load_resid: hipcc allocates the lambda form of this loop 17 registers worse in the
    //  7 x 3 kernel -- 68 bytes of scratch)
#pragma unroll
    for (int tm = 0; tm < CF::TM; ++tm) {
      mrow[tm] = row_of(tm * 32 + 8 * wave + row8);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        if (hilo_in) {
          const int64_t off = ((int64_t)max(mrow[tm], 0) * p.ldr16 + n0 + 32 * j + 4 * c8) * 2;
          const uint2 h2 = *reinterpret_cast<const uint2*>(p.resid_hi + off);
          const uint2 l2 = p.resid_lo != nullptr ? *reinterpret_cast<const uint2*>(p.resid_lo + off) : make_uint2(0u, 0u);   // hi only: a 16-bit stream
          rs[tm][j] = make_float4(__uint_as_float(h2.x), __uint_as_float(h2.y), __uint_as_float(l2.x), __uint_as_float(l2.y));
        } else {
          rs[tm][j] = *reinterpret_cast<const float4*>(p.resid + (int64_t)max(mrow[tm], 0) * p.ldr + n0 + 32 * j + 4 * c8);
        }
      }
    }
  } else {
#pragma unroll
    for (int tm = 0; tm < CF::TM; ++tm) {
      mrow[tm] = row_of(tm * 32 + 8 * wave + row8);
      if (tm < RS_FIRST) load_resid(tm);
    }
  }
  __syncthreads();                                                  // every wave's last fragment read has returned
  float4 b4[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j)
    b4[j] = p.bias != nullptr ? *reinterpret_cast<const float4*>(p.bias + n0 + 32 * j + 4 * c8) : make_float4(0.f, 0.f, 0.f, 0.f);
  float* cbase = reinterpret_cast<float*>(p.C);
  const int n_groups = p.N / CF::BN;
  // Block tm + 1 is parked in the other buffer BEFORE block tm is read back (one wave's LDS operations execute in
  // order, so the reads queue behind those writes): the barrier of an iteration then waits for writes issued a whole
  // block earlier instead of exposing write -> barrier -> read every time.  The other buffer is free: its last readers
  // (block tm - 1) had their data before they reached this iteration's barrier.
  auto park = [&](const int tm) {
    char* mine = smem + (tm & 1) * (4 * CF::PART_BYTES) + wave * CF::PART_BYTES;
#pragma unroll
    for (int tn = 0; tn < CF::TN; ++tn)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<float4*>(mine + l31 * CF::FROW + (tn * 32 + 8 * g + 4 * half) * 4) =
            make_float4(acc[tn][tm][4 * g], acc[tn][tm][4 * g + 1], acc[tn][tm][4 * g + 2], acc[tn][tm][4 * g + 3]);
  };
  park(0);
#pragma unroll
  for (int tm = 0; tm < CF::TM; ++tm) {
    char* buf = smem + (tm & 1) * (4 * CF::PART_BYTES);
    const int m = mrow[tm];
    __syncthreads();
    if (tm + 1 < CF::TM) park(tm + 1);
    if constexpr (RS_FIRST < CF::TM) {
      if (tm == 1) {                                                // blocks 0 .. 2 are parked: their registers are free
#pragma unroll
        for (int t2 = RS_FIRST; t2 < CF::TM; ++t2) load_resid(t2);
      }
    }
    float4 v[NJ];
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const char* src = buf + (8 * wave + row8) * CF::FROW + (32 * j + 4 * c8) * 4;
      const float4 p0 = *reinterpret_cast<const float4*>(src), p1 = *reinterpret_cast<const float4*>(src + CF::PART_BYTES);
      const float4 p2 = *reinterpret_cast<const float4*>(src + 2 * CF::PART_BYTES);
      const float4 p3 = *reinterpret_cast<const float4*>(src + 3 * CF::PART_BYTES);
      float4 r4 = rs[tm][j];
      if (hilo_in) {                                                // resid = hi + lo
        const float2 h01 = two16(__float_as_uint(r4.x)), h23 = two16(__float_as_uint(r4.y));
        const float2 l01 = two16(__float_as_uint(r4.z)), l23 = two16(__float_as_uint(r4.w));
        r4 = make_float4(h01.x + l01.x, h01.y + l01.y, h23.x + l23.x, h23.y + l23.y);
      }
      v[j].x = (((p0.x + p1.x) + (p2.x + p3.x)) + b4[j].x) + r4.x;
      v[j].y = (((p0.y + p1.y) + (p2.y + p3.y)) + b4[j].y) + r4.y;
      v[j].z = (((p0.z + p1.z) + (p2.z + p3.z)) + b4[j].z) + r4.z;
      v[j].w = (((p0.w + p1.w) + (p2.w + p3.w)) + b4[j].w) + r4.w;
      sum += (v[j].x + v[j].y) + (v[j].z + v[j].w);
    }
    if (m >= 0) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int n = n0 + 32 * j + 4 * c8;
        if (m >= p.c_row0) store_out16(reinterpret_cast<float4*>(cbase + (int64_t)m * p.ldc + n), v[j]);
        if (p.out2 != nullptr) {
          const uint2 hi = make_uint2(pack2<TAct>(v[j].x, v[j].y), pack2<TAct>(v[j].z, v[j].w));
          store_out8(reinterpret_cast<TAct*>(p.out2) + (int64_t)m * p.ldout2 + n, hi);
          if (p.out_lo != nullptr) {                                // lo = round16(v - hi): what hi dropped
            const float2 h01 = two16(hi.x), h23 = two16(hi.y);
            store_out8(reinterpret_cast<TAct*>(p.out_lo) + (int64_t)m * p.ldout2 + n,
                       make_uint2(pack2<TAct>(v[j].x - h01.x, v[j].y - h01.y), pack2<TAct>(v[j].z - h23.x, v[j].w - h23.y)));
          }
        }
      }
    }
    if (p.ln_stats != nullptr) {                                    // (mean, sum of squared deviations) over the 96 columns
      const float mean = row8_sum(sum) * (1.0f / CF::BN);
      float q = 0.f;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const float dx = v[j].x - mean, dy = v[j].y - mean, dz = v[j].z - mean, dw = v[j].w - mean;
        q += (dx * dx + dy * dy) + (dz * dz + dw * dw);
      }
      q = row8_sum(q);
      if (m >= 0 && c8 == 0) reinterpret_cast<float2*>(p.ln_stats)[(int64_t)m * n_groups + tile_n] = make_float2(mean, q);
    }
  }
#ifdef RPO_TIMELINE
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
  RPO_STAMP(61); RPO_STAMP_RT(63);
}

template <typename TAct, typename CF>
__global__ __launch_bounds__(256, 1) void gemm_w4k_kernel(const GemmParams p, const int rows0, const int rows1,
                                                          const int seg1_base, const int tiles_n) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  gemm_w4k_body<TAct, CF>(p, rows0, rows1, seg1_base, tiles_n, smem);
}

// Applies when the caller's row units (rpo_gemm_args.seg_*) give whole rounds of tiles: BIAS_RESID, 16-bit A / W, fp32 C,
// N a multiple of the tile width, an admitted number of k-tiles, and statistics (if any) over tile-width column groups.
template <typename CF>
static inline bool w4k_plan_t(const GemmParams& p, W4RowsPlan* q) {
  if (p.K % CF::BK != 0) return false;
  const int nk = p.K / CF::BK;
  if (nk < CF::RING) return false;
  if constexpr (CF::RING == 4) { if (nk % 4 != 0) return false; }          // loop entered at position 0 only
  else { if (nk % 6 != 0 && nk % 6 != 4) return false; }                   // entry positions 3 / 5 (tools/gen_gemm_w4.py)
  return w4_unit_plan<CF>(p, q);
}
// 0: no geometry applies; else the statistics group width (= tile width) of the geometry that does: 96 or 64
// (q->geo = its TM: 7, 8 or 9)
static inline int w4k_plan(const GemmParams& p, W4RowsPlan* q) {
  if (w4k_plan_t<CfgW4K>(p, q)) return CfgW4K::BN;
#ifndef RPO_W4K_NO_8X3
  if (w4k_plan_t<CfgW4K8>(p, q)) return CfgW4K8::BN;
#endif
  if (w4k_plan_t<CfgW4KL>(p, q)) return CfgW4KL::BN;
  return 0;
}

template <typename TAct>
int launch_w4k(const GemmParams& p, hipStream_t s) {
  W4RowsPlan q;
  if (w4k_plan(p, &q) == 0) return RPO_E_SHAPE;
  switch (q.geo) {
    case CfgW4K::TM: return launch_w4_rows<gemm_w4k_kernel<TAct, CfgW4K>, CfgW4K>(p, q, s);
    case CfgW4K8::TM: return launch_w4_rows<gemm_w4k_kernel<TAct, CfgW4K8>, CfgW4K8>(p, q, s);
    case CfgW4KL::TM: return launch_w4_rows<gemm_w4k_kernel<TAct, CfgW4KL>, CfgW4KL>(p, q, s);
    default: return RPO_E_SHAPE;
  }
}
