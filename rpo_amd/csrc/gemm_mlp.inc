// gemm_mlp.inc -- included by gemm.hip inside its anonymous namespace, after gemm_w4k.inc.
//
// ---- c_fc -> c_proj of an image block as ONE launch (round 4, EXPERIMENT: rpo_mlp_fused, opt-in RPO_MLP_FUSED=1) -----
// The round-3 review's "stage A" of the per-image workgroup groups: with row units the 8 workgroups that own one image's
// column tiles in c_fc (224 x 384 tiles, gemm_w4g.inc) are the 8 that own its column tiles in c_proj (224 x 96 tiles,
// gemm_w4k.inc), and they sit on one XCD (block b runs on XCD b % 8, an XCD takes whole row units).  Here a workgroup runs
// the c_fc body, waits for the other 7 of its image at a counter, and runs the c_proj body: one kernel boundary (and its
// write-back of the 44 MB of g) less per block, g read out of the XCD's L2 instead of the memory-side cache.
//
// Hand-off.  Producer side: every wave drains its own stores (s_waitcnt vmcnt(0): they have reached the L2), workgroup
// barrier, thread 0 adds 1 to the image's counter (agent-scope relaxed atomic; returns the old value v) and polls until
// the counter reaches (v / 8 + 1) * 8 -- launches are stream-ordered, so the 8 arrivals of one launch share v / 8 and the
// counters never need resetting (graph replays re-use the arguments).  Consumer side: the c_proj body's first reads of g
// are this CU's first touches of those lines in this launch (the L1 was invalidated at kernel start), so they are served
// by the L2 the producers wrote to -- IF all 8 share that L2.  `safe` != 0 does not rely on it: agent-scope release
// before the arrive, agent-scope acquire after the poll (placement-independent, the form of MI355X_MICROARCH.md).
// The launcher admits the kernel only when every workgroup is resident at once (units * 8 <= CUs, one per CU: 160 KiB of
// LDS): a workgroup that has not started cannot be waited for (and every poll is bounded: counters[units] counts give-ups).
template <typename T, int EPI_FC>
__global__ __launch_bounds__(256, 1) void mlp_fused_kernel(const GemmParams pf, const GemmParams pp, const int rows0,
                                                          const int rows1, const int seg1_base, unsigned int* counters,
                                                          const int safe) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tn_fc = pf.N / CfgW4G::BN, tn_proj = pp.N / CfgW4K::BN;      // both 8: the launcher checks
  gemm_w4g_body<T, EPI_FC, CfgW4G>(pf, rows0, rows1, seg1_base, tn_fc, smem);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                       // this wave's stores of g (and u) are in the L2
  __syncthreads();                                                       // ... everybody's; c_fc's LDS staging is dead
  if (threadIdx.x == 0) {
    const int nwg = gridDim.x, bid = blockIdx.x;
    const int tile_m = xcd_run(bid, nwg) / tn_fc;                      // the row unit, as in the two bodies
    if (safe) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    unsigned int* c = counters + tile_m;
    const unsigned int old = __hip_atomic_fetch_add(c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned int want = (old / (unsigned)tn_fc + 1u) * (unsigned)tn_fc;
    // bounded (~10 s): a workgroup that can never arrive -- a grid that is not resident at once -- must not hang the device;
    // a give-up is counted in counters[units] (the caller checks: results are then invalid)
    unsigned int spins = 0;
    while ((int)(__hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - want) < 0) {
      __builtin_amdgcn_s_sleep(2);
      if (++spins > (1u << 24)) {
        __hip_atomic_fetch_add(counters + gridDim.x / tn_fc, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
    }
    if (safe) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  }
  __syncthreads();
  gemm_w4k_body<T, CfgW4K>(pp, rows0, rows1, seg1_base, tn_proj, smem);
}

template <typename T, int EPI_FC>
int launch_mlp_fused(const GemmParams& pf, const GemmParams& pp, const W4RowsPlan& g, unsigned int* counters, int safe, hipStream_t s) {
  static rpo_lds_mask_t lds_ok{0};
  auto kern = mlp_fused_kernel<T, EPI_FC>;
  constexpr int bytes = CfgW4G::SMEM > CfgW4K::SMEM ? CfgW4G::SMEM : CfgW4K::SMEM;
  if (int rc = rpo_allow_lds(reinterpret_cast<const void*>(kern), bytes, &lds_ok)) return rc;
  hipLaunchKernelGGL(kern, dim3(g.tiles_m * g.tiles_n, 1), dim3(256), bytes, s, pf, pp, g.rows0, g.rows1, g.seg1_base,
                     counters, safe);
  return rpo_launch_status();
}
