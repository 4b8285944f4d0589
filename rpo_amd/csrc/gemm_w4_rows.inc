// gemm_w4_rows.inc -- included by gemm.hip inside its anonymous namespace, before gemm_w4g.inc and gemm_w4k.inc: the host
// side the two row-unit kernels share -- the plan of one tile per row unit and the launcher.
//
// The device-side prologues of gemm_w4g_body and gemm_w4k_body (row_of, the DMA offsets and descriptors, the accumulator
// zeroing) are the same text and stay two copies: moved into a shared struct or function -- by value, by reference, with
// the row lookup passed in as a closure, or only the zeroing loop as a function over the accumulator array -- hipcc
// emits the same instructions in another order or with other registers around the k-loops, first of all in the two
// LayerNorm-fold instantiations of the 224x384 geometry, the ones one live VGPR away from spilling.  What they do share is
// xcd_run (gemm.hip) and the generated operand lists (gemm_w4?_asm.inc).

// one workgroup per CU and round: the tile count must fill (most of) a whole number of rounds of the 256 CUs -- one round
// at 32 images, two at 64, four at 128
static inline bool w4_rounds_ok(int tiles) {
  const int rounds = (tiles + 255) / 256;
#ifndef RPO_W4_MINFILL
#define RPO_W4_MINFILL 81
#endif
  return rounds >= 1 && rounds <= 8 && tiles * 100 >= rounds * 256 * RPO_W4_MINFILL;
}
// from_units: one tile = one of the caller's row units (rpo_gemm_args.seg_*); geo = TM of the geometry
struct W4RowsPlan { int rows0, rows1, seg1_base, tiles_m, tiles_n; bool from_units; int geo; };
// One tile per row unit, if the caller gave units that fit the geometry CF and the tiles make whole rounds
template <typename CF>
static inline bool w4_unit_plan(const GemmParams& p, W4RowsPlan* q) {
  if (p.N % CF::BN != 0 || p.seg_rows0 <= 0 || p.seg_rows0 + p.seg_rows1 > CF::BM || p.seg1_row0 % p.seg_rows0 != 0) return false;
  const int tn = p.N / CF::BN, units = p.seg1_row0 / p.seg_rows0;
  if (p.M - p.seg1_row0 != units * p.seg_rows1 || !w4_rounds_ok(units * tn)) return false;
  *q = W4RowsPlan{p.seg_rows0, p.seg_rows1, p.seg1_row0, units, tn, true, CF::TM};
  return true;
}

template <auto Kernel, typename CF>
int launch_w4_rows(const GemmParams& p, const W4RowsPlan& q, hipStream_t s) {
  static rpo_lds_mask_t lds_ok{0};
  if (int rc = rpo_allow_lds(reinterpret_cast<const void*>(Kernel), CF::SMEM, &lds_ok)) return rc;
  hipLaunchKernelGGL(Kernel, dim3(q.tiles_m * q.tiles_n, 1), dim3(CF::THREADS), CF::SMEM, s, p, q.rows0, q.rows1,
                     q.seg1_base, q.tiles_n);
  return rpo_launch_status();
}
