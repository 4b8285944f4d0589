/*
 * rpo_amd.h -- C ABI of librpo_hip.so: the MI355X (gfx950) kernels behind RPO's
 * few-shot train step.
 *
 * The reference (mlvlab/RPO) has no FFI / plugin registry: its hot path is stock
 * torch.nn modules called from trainers/rpo.py:161-232 (CustomCLIP.forward) and
 * clip/model.py:181-207 (ResidualAttentionBlock / Transformer).  Each entry point
 * below replaces one stock-torch op sequence on that path; the comment on each
 * cites the reference lines it stands in for.  INTEGRATION.md shows the ctypes
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *   - plain pointers + sizes only; every pointer is a DEVICE pointer unless noted
 *   - the caller (PyTorch-ROCm) allocates and owns every buffer; nothing here
 *     allocates, frees or keeps state a caller could observe (the one internal cache: an atomic per-kernel
 *     "large-LDS attribute already set on device d" bit in front of an idempotent hipFuncSetAttribute)
 *   - every function only ENQUEUES work on `stream` (a hipStream_t passed as
 *     void*; 0 = the null stream) and returns immediately
 *   - return value: 0 = ok, > 0 = hipError_t of the launch, < 0 = RPO_E_* argument
 *     error (nothing was enqueued); rpo_error_string() decodes any of them
 *   - dtype arguments take RPO_F32 / RPO_BF16 / RPO_F16.  "act dtype" is the storage type of
 *     activations and frozen weights: RPO_F32 = parity mode (exact-f32 MFMA,
 *     v_mfma_f32_32x32x2_f32), RPO_BF16 = throughput mode (bf16 storage,
 *     v_mfma_f32_32x32x16_bf16, fp32 accumulate).  The residual stream, LayerNorm
 *     statistics, softmax, logits, loss, gradients of the prompts and the
 *     optimiser state are fp32 in both modes.
 *   - leading dimensions (ld*) are in ELEMENTS of the respective dtype
 *
 * Row layout of the image tower (B images, N = 1 + patches frozen tokens,
 * Kp read-only prompts per image):
 *     rows [0, B*N)          frozen tokens, image-major:  b*N + t
 *     rows [B*N, B*N + B*Kp) prompt tokens, image-major:  B*N + b*Kp + i
 * so the rows that are back-propagated form one contiguous sub-matrix.
 */
#ifndef RPO_AMD_H
#define RPO_AMD_H

#include <stddef.h>
#include <stdint.h>

/* The library is built with -fvisibility=hidden: only what this header declares is exported. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif
#ifdef __cplusplus
extern "C" {
#endif

#define RPO_ABI_VERSION 8

enum { RPO_F32 = 0, RPO_BF16 = 1, RPO_F16 = 2 };

enum {
  RPO_E_BADARG = -1,   /* null pointer / non-positive size */
  RPO_E_SHAPE = -2,    /* size not supported by the kernels (see each function) */
  RPO_E_DTYPE = -3,    /* dtype combination not supported */
  RPO_E_ALIGN = -4,    /* pointer / leading dimension not 16-byte aligned */
  RPO_E_WORKSPACE = -5, /* caller-provided workspace / table bounds too small for this call */
  /* rpo_jpeg_probe: the file is not one the device decodes (the caller decodes it on the host instead) */
  RPO_E_JPEG_CORRUPT = -20,     /* not a JPEG, or a header that is truncated / inconsistent */
  RPO_E_JPEG_PROGRESSIVE = -21, /* SOF2 and the other progressive frames */
  RPO_E_JPEG_ARITHMETIC = -22,  /* arithmetic coding */
  RPO_E_JPEG_LOSSLESS = -23,    /* lossless / hierarchical frames */
  RPO_E_JPEG_PRECISION = -24,   /* 12-bit samples, or 16-bit quantisation tables */
  RPO_E_JPEG_COMPONENTS = -25,  /* not 1 or 3 components (CMYK / YCCK) */
  RPO_E_JPEG_RGB = -26,         /* RGB-coded: Adobe APP14 transform 0, or component ids 'R','G','B' */
  RPO_E_JPEG_SAMPLING = -27,    /* sampling other than 4:4:4, 4:2:2 (h2v1), 4:2:0 (h2v2) */
  RPO_E_JPEG_MULTISCAN = -28,   /* the first scan does not hold every component */
  /* rpo_jpeg_prog_probe only */
  RPO_E_JPEG_SCRIPT = -29,      /* progressive scan script incomplete, inconsistent or otherwise outside the accepted rules */
  RPO_E_JPEG_SEQUENTIAL = -30   /* a sequential (SOF0 / SOF1) frame: rpo_jpeg_probe is the one that handles it */
};

/* GEMM epilogues (fused into the MFMA kernel's store) */
enum {
  RPO_EPI_NONE = 0,        /* C = acc                                  (dX GEMMs of the backward)            */
  RPO_EPI_BIAS = 1,        /* C = acc + bias[n]                        (in-proj, clip/model.py:186)          */
  RPO_EPI_BIAS_QGELU = 2,  /* C = quickgelu(acc + bias); optionally saves u = acc + bias (fp32) for rows
                              >= aux_row0 (the rows that will be back-propagated)   (c_fc, clip/model.py:174-175) */
  RPO_EPI_BIAS_RESID = 3,  /* C(f32) = resid + acc + bias              (out_proj / c_proj + residual, :189-190) */
  RPO_EPI_QGELU_BWD = 4,   /* C = acc * quickgelu'(aux[m,n])           (backward through clip/model.py:162-164) */
  RPO_EPI_PATCH = 5,       /* C(f32)[m + m/group + 1, n] = acc + resid[(m % group) + 1, n]: patch embedding
                              written straight into the token matrix with the positional embedding added
                              (trainers/rpo.py:198-202)                                                      */
  /* LayerNorm folded into the GEMM that consumes it (clip/model.py:156-159 feeding :186 / :174).  With
     W'[n,k] = gamma[k] W[n,k], s[n] = sum_k W'[n,k], b'[n] = b[n] + sum_k beta[k] W[n,k]:
         LN(x) . W^T + b  =  rstd[m] * (x . W'^T - mu[m] * s[n]) + b'[n]
     so A is the RAW residual row (16-bit copy written by the producing GEMM, `out2` below), W = W', bias = b',
     ln_colsum = s, and mu / rstd come from the per-row partial statistics the producer left in ln_stats.
     Limit: A is x rounded to the act dtype, so a row whose spread is far below the act-dtype ulp of its mean (a
     near-constant row: sigma 1e-4 at mean 3) loses its variation before the GEMM; the unfolded LayerNorm reads fp32 x.
     Rows with channels in the hundreds or means up to 50 sigma stay within the unfolded path's tolerance. */
  RPO_EPI_LN_BIAS = 6,       /* C = LN-fold(acc)                        (ln_1 + in-proj)                     */
  RPO_EPI_LN_BIAS_QGELU = 7  /* C = quickgelu(LN-fold(acc)), aux as BIAS_QGELU   (ln_2 + c_fc)               */
};

typedef struct rpo_gemm_args {
  const void* A;  int64_t lda;   /* [M, K] act dtype, row-major                                   */
  const void* W;  int64_t ldw;   /* [N, K] act dtype, row-major (nn.Linear weight layout [out,in]) */
  void* C;        int64_t ldc;   /* [M, N] out_dtype                                              */
  int32_t M, N, K;
  int32_t in_dtype, out_dtype, epilogue;
  const float* bias;             /* [N] fp32 or NULL                                              */
  const float* resid; int64_t ldr; /* fp32; RESID: [M, N]; PATCH: positional embedding [group+1, N] */
  void* aux; int64_t ldaux;      /* fp32; see epilogues                                           */
  int32_t aux_row0;              /* BIAS_QGELU: first row whose pre-activation is saved (aux row 0);
                                    pass M (or aux = NULL) to save nothing                        */
  int32_t skip_row0, skip_col0;  /* tiles with all rows >= skip_row0 AND all cols >= skip_col0 are not
                                    computed (K/V of prompt rows are never read); -1 disables      */
  int32_t group;                 /* PATCH: patches per image                                       */
  int32_t split_k;               /* <= 1: off.  S > 1 (EPI_NONE, fp32 C only): k-range split into S slices,
                                    slice s writes its partial product to C + s * split_stride; the
                                    consumer (rpo_layernorm_bwd's dy_splits) adds the slabs in order    */
  int64_t split_stride;          /* elements between slabs (>= M * ldc)                            */
  int32_t tile_config;           /* 0 = choose by shape.  For benchmarking / tests (a config whose conditions do not hold falls
                                    through to the shape heuristic unless noted): 2 = 128x128 tiles, 5 = 64x64, 6 = 64x128,
                                    9 = 128x128 with 4 waves; 16-bit in / out with a BIAS-type or LN epilogue: 3 = 256x256
                                    lock-step, 7 = 256x256 ping-pong, 8 = 256x256 one wave per SIMD (what 0 picks when the
                                    tiles fill a round of the CUs), 10 = 224x384 (N % 384 == 0) or 288x256 (N % 256 == 0)
                                    tiles in whole rounds of the CUs (what 0 picks for c_fc at 32 / 64 / 128 images of
                                    ViT-B/16, 16 of ViT-L/14); BIAS_RESID, 16-bit in, fp32 out: 11 = 224x96 or 288x64
                                    tiles with the waves splitting k (needs the row-unit hint below; RPO_E_SHAPE if it
                                    does not apply).  Configs 2 / 3 / 5 / 6 / 7 / 8 / 9 / 10 give bit-identical results;
                                    11 sums k in four parts and differs in the last bits                              */
  /* LayerNorm fold (all optional, 0 / NULL = off) */
  void* out2; int64_t ldout2;    /* BIAS_RESID: also store C in the act dtype (in_dtype) here: the A operand of the
                                    GEMM that consumes LN(C)                                        */
  float* ln_stats;               /* BIAS_RESID: OUT, [M][N/g][2] fp32: (mean, sum of squared deviations) of every
                                    g-column group of the row of C just written, g = ln_group (64 or 96).
                                    LN_BIAS*: IN, the same array for the rows of A (groups = K / g <= 16) */
  const float* ln_colsum;        /* LN_BIAS*: s[n], fp32 [N]                                         */
  float ln_eps;                  /* LN_BIAS*: epsilon of the folded LayerNorm                        */
  /* Optional tiling hint (results do not depend on it): the rows of A / C are two segments, [0, seg1_row0) and
     [seg1_row0, M), and unit u owns rows [u * seg_rows0, +seg_rows0) of the first and [seg1_row0 + u * seg_rows1,
     +seg_rows1) of the second -- the image tower's layout: N frozen rows + Kp prompt rows per image.  A kernel that
     tiles one unit per workgroup then spreads the rows with extra epilogue work (saved pre-activations) evenly. */
  int32_t seg_rows0, seg_rows1, seg1_row0;
  /* Columns per partial row statistic in ln_stats: 0 or 64 (default), or 96.  96 is what the one-round 224x96 kernel
     writes (BIAS_RESID with a row-unit hint, N % 96 == 0, K % 256 == 0: tile_config 11 / the heuristic's choice for the
     image tower's out-proj and c_proj of ViT-B/16; its 288x64 geometry for ViT-L/14 writes 64); a producer that cannot
     write the requested layout returns RPO_E_SHAPE, and the consuming LN_BIAS* GEMM must be given the same value.
     rpo_gemm_stats_group() tells which. */
  int32_t ln_group;
  /* What aux holds.  RPO_F32 (0, default): the fp32 pre-activation u -- *_QGELU epilogues write it, QGELU_BWD evaluates
     quickgelu'(u).  in_dtype (16-bit modes only): d quickgelu / du itself in the act dtype ([rows, ldaux] of that type) --
     *_QGELU epilogues write it, QGELU_BWD multiplies by it: half the bytes, no transcendental in the backward. */
  int32_t aux_dtype;
  /* Optional hint (results do not depend on it; may be NULL): `prefetch_bytes` bytes at `prefetch` are what the NEXT
     launch on this stream will read first -- in the image tower the next GEMM's frozen weight matrix, which no cache
     still holds a whole step after its last use.  The one-round kernels have every workgroup touch its 1 / grid share
     of those lines (one dword per 128-B line, issued before the k-loop) so that the next kernel finds them in the
     memory-side cache instead of HBM.  Kernels that do not implement the hint ignore it. */
  const void* prefetch;
  int64_t prefetch_bytes;
  /* Residual stream as 16-bit hi / lo halves (BIAS_RESID, 16-bit inputs, optional; ABI 4).  The fp32 residual stream of
     a transformer block (clip/model.py:188-190: x = x + attn(ln_1(x)); x = x + mlp(ln_2(x))) is written and re-read in
     full by every residual GEMM, next to the 16-bit copy the following GEMM consumes.  With these fields the stream lives
     as hi = round16(v) -- which IS that copy (out2) -- and lo = round16(v - hi): resid_hi / resid_lo replace `resid` as
     the input (leading dimension ldr16, in elements; resid_lo may be NULL: the stream is then the 16-bit hi alone, which
     is what the reference's own `PREC: fp16` run keeps -- clip/model.py:379-400 converts the model, :153-159 casts
     LayerNorm's fp32 result back), out_lo receives lo next to out2 (leading dimension ldout2; NULL: not kept), and the fp32 C is stored only for rows >= c_row0 (the back-propagated rows, whose LayerNorm backward reads
     fp32; pass 0 to store all rows).  hi + lo carries 16 mantissa bits (bf16) / 22 (fp16) of the fp32 value.  In place is
     allowed (resid_hi == out2, resid_lo == out_lo: every element is read and written by the same thread).  Only the
     one-round row-unit kernels implement it: rpo_gemm_hilo_ok() tells; anything else returns RPO_E_SHAPE. */
  const void* resid_hi; const void* resid_lo; int64_t ldr16;
  void* out_lo;
  int32_t c_row0;
} rpo_gemm_args;

int rpo_version(void);
const char* rpo_error_string(int code);

/* C = A . W^T with a fused epilogue.  Requires K % 64 == 0 (bf16) / K % 32 == 0 (f32),
 * N % 4 == 0, 16-byte aligned rows.  Replaces nn.Linear / F.linear / the matmuls of
 * nn.MultiheadAttention's packed in-proj and out-proj (clip/model.py:171-177,186) and,
 * in the backward, autograd's mm(dY, W) (trainers/rpo.py:308). */
int rpo_gemm_nt(const rpo_gemm_args* args, void* stream);

/* ---- rpo_gemm_nt for the PROMPT ROWS: a few hundred rows against a frozen weight (ABI 7) -------------------------------
 * Same contract as rpo_gemm_nt (C = A . W^T with the fused epilogues above; replaces nn.Linear's matmul,
 * clip/model.py:173-177,186, and autograd's mm(dY, W), trainers/rpo.py:308, for the B*K / n_cls*K prompt rows of the
 * two towers), except that W is the FRAGMENT-MAJOR copy rpo_gemm_ws_pack made of the [N, K] weight once at load time:
 * the weight operand then streams global -> VGPR in MFMA fragment order (1 KiB per wave-instruction, no LDS), the four
 * waves of a workgroup split the contraction, and the tile (32x32 .. 96x96) is chosen so that the launch covers the CUs
 * about once (rpo_amd/csrc/gemm_ws.hip).  args->W = the packed copy, args->ldw is ignored.
 *   16-bit inputs only (RPO_E_DTYPE otherwise); K % 64 == 0, N % 32 == 0; epilogues NONE (16-bit or fp32 C; split_k slabs
 *   as rpo_gemm_nt), QGELU_BWD, BIAS, BIAS_QGELU, LN_BIAS, LN_BIAS_QGELU (K / ln_group <= 16), BIAS_RESID (fp32 C;
 *   out2 / ln_stats over 64-column groups); no skip_*, row units or hi / lo residual (RPO_E_SHAPE: use rpo_gemm_nt).
 *   tile_config: 0 = choose; 100 * MT + 10 * NT forces MT x NT MFMA tiles per workgroup (110, 120, 220, 330).
 * Deterministic; the k sum is split in four, so the last bits differ from rpo_gemm_nt's. */
int rpo_gemm_ws(const rpo_gemm_args* args, void* stream);
/* Wp[N * K] (act dtype, 16-byte aligned) <- W[N, K] row-major (ldw in elements): piece ((nb * K/16 + ks) * 64 + lane) of 8
 * elements = W[nb * 32 + (lane & 31)][ks * 16 + (lane >> 5) * 8 ..].  N % 32 == 0, K % 64 == 0. */
int rpo_gemm_ws_pack(const void* W, int64_t ldw, void* Wp, int N, int K, int dtype, void* stream);
/* 1 if rpo_gemm_ws takes these shapes / dtypes / epilogue (pointers are not looked at), else 0 */
int rpo_gemm_ws_ok(const rpo_gemm_args* args);

/* The partial-statistics layout (rpo_gemm_args.ln_group: 64 or 96) a BIAS_RESID producer writes for these shapes,
 * dtypes and row units when the kernel choice is left to the library (tile_config 0).  Only M, N, K, lda, ldw, the
 * dtypes, split_k and seg_* are looked at.  Callers size ln_stats as [M, N / group, 2] floats and pass the same group to
 * the producer and to the LN_BIAS* consumer. */
int rpo_gemm_stats_group(const rpo_gemm_args* args);

/* 1 if rpo_gemm_nt would run these shapes / dtypes / row units on a kernel that implements the hi / lo residual stream
 * (resid_hi, resid_lo, out_lo, c_row0 above), else 0.  Looks at the same fields as rpo_gemm_stats_group plus ln_group. */
int rpo_gemm_hilo_ok(const rpo_gemm_args* args);

/* What rpo_gemm_nt would do with these arguments, without launching anything: the tile_config value that forces the
 * kernel it would run (> 0: 5 = 64x64, 6 = 64x128, 2 = 128x128, 9 = 128x128 with 4 waves, 3 / 7 / 8 = 256x256,
 * 10 = 224x384 / 288x256 row-unit tiles, 11 = 224x96 / 256x96 / 288x64 split-k tiles), or the negative RPO_E_* it would
 * return.  Same argument checks and the same choice as the call (one code path); pointers are checked, not dereferenced.
 * A launch error (> 0 from the call) is not predicted. */
int rpo_gemm_nt_plan(const rpo_gemm_args* args);
/* The same for rpo_gemm_ws: its geometry as the tile_config code 100 * MT + 10 * NT (> 0), or the RPO_E_* it would return. */
int rpo_gemm_ws_plan(const rpo_gemm_args* args);

/* y = LayerNorm(x) * gamma + beta, statistics in fp32, eps as given (1e-5).
 * x fp32 [rows, d] (ldx), y in y_dtype.  d % 4 == 0, d <= 2048.  In-place (y == x, fp32) is allowed.
 * Replaces clip/model.py:153-159 (ln_1, ln_2, ln_pre, ln_post, ln_final). */
int rpo_layernorm_fwd(const float* x, int64_t ldx, const float* gamma, const float* beta,
                      void* y, int64_t ldy, int y_dtype, int rows, int d, float eps, void* stream);

/* dx = dres + dLN(dy; x, gamma)   (frozen affine: no dgamma/dbeta).
 * dy in dy_dtype [rows, d] -- or, with dy_splits = S > 1 (fp32 only), the sum of S slabs
 * dy + s * dy_split_stride written by a split-K rpo_gemm_nt, added in the order s = 0..S-1;
 * x fp32 = the forward input; dres fp32 or NULL;
 * dx fp32; dx_cast (optional, may be NULL) receives a copy of dx in cast_dtype
 * (the next GEMM's A operand).  Replaces autograd through clip/model.py:158. */
int rpo_layernorm_bwd(const void* dy, int dy_dtype, int64_t lddy, const float* x, int64_t ldx,
                      const float* gamma, const float* dres, int64_t lddres,
                      float* dx, int64_t lddx, void* dx_cast, int cast_dtype, int64_t ldcast,
                      int rows, int d, float eps, int dy_splits, int64_t dy_split_stride, void* stream);

/* Non-overlapping-patch im2col: img [B,3,H,W] fp32 -> out [B*(H/p)*(W/p), ldo] act dtype, column
 * order (c, ky, kx) = conv1.weight.reshape(d, -1); columns [3*p*p, ldo) are zero-filled.
 * With rpo_gemm_nt(RPO_EPI_PATCH) this replaces the stride-p Conv2d at trainers/rpo.py:198-200. */
int rpo_im2col_patches(const float* img, void* out, int out_dtype, int64_t ldo,
                       int B, int H, int W, int patch, void* stream);

/* Writes the rows the patch GEMM does not: CLS rows x[b*N] = cls + pos[0] and the prompt rows
 * x[B*N + b*Kp + i] = img_prompt[i] (no positional embedding: trainers/rpo.py:201-204). */
int rpo_img_assemble(float* x, int64_t ldx, const float* cls, const float* pos0,
                     const float* img_prompt, int B, int N, int Kp, int d, void* stream);

/* rpo_img_assemble + ln_pre + the first block's ln_1 in one launch (trainers/rpo.py:201-206, clip/model.py:189): per
 * token row -- CLS + pos[0], the patch row already in x_pre, or the image's prompt row -- x0 = ln_pre(token) (fp32) and
 * h = ln_1(x0) (h_dtype).  The CLS and prompt rows are also written to x_pre (the backward of ln_pre reads the prompt
 * rows).  Same bits as the three separate launches.  d % 4 == 0, d <= 1024. */
int rpo_img_embed_norm(float* x_pre, int64_t ldx, const float* cls, const float* pos0, const float* img_prompt,
                       const float* g_pre, const float* b_pre, float* x0, int64_t ldx0, const float* g1, const float* b1,
                       void* h, int64_t ldh, int h_dtype, int B, int N, int Kp, int d, float eps, void* stream);
/* (ABI 8) The same for the token rows [row0, row1) only.  The frozen rows [0, B*N) depend on the batch alone, not on the
 * prompts (trainers/rpo.py:198-203), so a trainer may form them for the NEXT batch while this step's backward is still
 * running and run [B*N, B*(N+Kp)) -- the prompt rows -- at the head of the next image forward.  Row by row the bits of
 * rpo_img_embed_norm. */
int rpo_img_embed_norm_rows(float* x_pre, int64_t ldx, const float* cls, const float* pos0, const float* img_prompt,
                            const float* g_pre, const float* b_pre, float* x0, int64_t ldx0, const float* g1,
                            const float* b1, void* h, int64_t ldh, int h_dtype, int B, int N, int Kp, int d,
                            float eps, int row0, int row1, void* stream);

/* (ABI 8 addition) The same with one prompt set per GROUP of images: set g = img_prompt + g * prompt_stride ([Kp, d] each,
 * prompt_stride in floats, >= Kp * d and a multiple of 4), and image b takes its prompt rows from set b / images_per_group
 * -- several RPO runs (trainers/rpo.py:201-204 once per run) sharing one pass over the frozen image tower.  Row by row the
 * bits of rpo_img_embed_norm_rows called with that set's prompt; images_per_group = B is that call.
 * B % images_per_group != 0, or overlapping sets (prompt_stride < Kp * d): RPO_E_SHAPE; a prompt_stride that is not a
 * multiple of 4 floats: RPO_E_ALIGN (with one set the stride is not looked at). */
int rpo_img_embed_norm_grouped(float* x_pre, int64_t ldx, const float* cls, const float* pos0, const float* img_prompt,
                               const float* g_pre, const float* b_pre, float* x0, int64_t ldx0, const float* g1,
                               const float* b1, void* h, int64_t ldh, int h_dtype, int B, int N, int Kp, int d,
                               float eps, int row0, int row1, int images_per_group, int64_t prompt_stride, void* stream);

/* dst[g*rows + i, :] = src[i, :]  (text prompts written into every class, trainers/rpo.py:176-177) */
int rpo_broadcast_rows(const float* src, float* dst, int64_t ld, int groups, int rows, int d, void* stream);

/* out[i, :] = sum_g src[g*rows + i, :] in fixed order g = 0..groups-1 (autograd of .repeat()) */
int rpo_reduce_groups(const float* src, int64_t ld, float* out, int groups, int rows, int d, void* stream);

/* (ABI 8 additions) Both for `sets` prompt sets in one launch each (several RPO runs in one step):
 *   dst[(s*groups + g)*rows + i, :] = src[s * src_set_stride + i * d ...]  set s of src: [rows, d] at s * src_set_stride
 *   out[s * out_set_stride + i * d ...] = sum_g src[(s*groups + g)*rows + i, :]
 * (strides in floats: the sets may be rows of a wider parameter / gradient buffer) with g in the order (and on the kernel) rpo_reduce_groups uses for `groups`: per set the bits of the plain calls on the
 * set's slices.  sets = 1 is the plain call. */
int rpo_broadcast_rows_sets(const float* src, int64_t src_set_stride, float* dst, int64_t ld, int sets, int groups, int rows,
                            int d, void* stream);
int rpo_reduce_groups_sets(const float* src, int64_t ld, float* out, int64_t out_set_stride, int sets, int groups, int rows,
                           int d, void* stream);

/* (ABI 8 addition) Input rows of a text pass, gathered on the device (make_prompts, trainers/rpo.py:135-136; CoOp's context
 * slots, trainers/coop.py:136-183): for c < n, p < L
 *   out[c * L + p, :] = table[ids[c * ld_ids + p], :] + pos[p, :]      for an id >= 0
 *   out[c * L + p, :] = ctx[-1 - id, :] + pos[p, :]                    for an id < 0 (context slot -1 - id)
 * ids int32 [n, ld_ids] (only the first L of a row are read), table [vocab, d], pos [>= L, d], ctx [n_ctx, d] or NULL when
 * n_ctx == 0, out [n * L, d] contiguous; all fp32 device memory, row indices 64-bit.  One fp32 add per element: the bits
 * of the host expression.  The caller validates ids; the kernel clamps an id into [0, vocab) / a slot into [0, n_ctx)
 * (a negative id with n_ctx == 0 reads row 0 of table), so no id reads outside the arguments.
 * A null pointer, n < 1, L < 1, vocab < 1, n_ctx < 0: RPO_E_BADARG; d % 4 != 0 or L > ld_ids: RPO_E_SHAPE; table, pos, ctx
 * or out not 16-byte aligned: RPO_E_ALIGN -- all with nothing launched.  One launch on `stream`, no allocation,
 * capturable in a HIP graph. */
int rpo_text_embed(const int32_t* ids, int64_t ld_ids, const float* table, int vocab, const float* pos, const float* ctx,
                   int n_ctx, float* out, int n, int L, int d, void* stream);

/* Read-only masked attention of the image tower, all heads (head_dim 64), all B images.
 * q, k, v: act-dtype matrices in the row layout above with leading dimension ld (typically
 * three column slices of one packed [R, 3d] in-proj output).  Every query row (frozen and
 * prompt) reads ONLY the N frozen keys of its own image: the additive mask of
 * trainers/rpo.py:154-156 is -inf on the prompt columns for all rows, so those columns are
 * skipped, not computed.  out[R, ldo] act dtype.  N <= 1025: up to 288 keys an image's K / V sit
 * in LDS at once; above that the keys are walked in chunks of 256 under an online softmax
 * (ViT-L/14 at 336 px: N = 577), and N > 1025 returns RPO_E_SHAPE with nothing launched.
 * Replaces F.scaled_dot_product_attention inside nn.MultiheadAttention (clip/model.py:186). */
int rpo_attn_readonly_fwd(const void* q, const void* k, const void* v, int64_t ld,
                          void* out, int64_t ldo, int dtype, int B, int H, int N, int Kp,
                          float scale, void* stream);
/* Same, computing only the queries q_first .. N+Kp-1 of every image (earlier rows of `out` are left untouched).  The
 * last block of the image tower needs the prompt queries only: ln_post reads nothing else (trainers/rpo.py:210).
 * N <= 1025, as above; a query's bits do not depend on q_first. */
int rpo_attn_readonly_fwd_rows(const void* q, const void* k, const void* v, int64_t ld,
                               void* out, int64_t ldo, int dtype, int B, int H, int N, int Kp, float scale,
                               int q_first, void* stream);

/* (ABI 8 addition) The prompt queries of `sets` prompt sets over SHARED frozen keys / values: the prompt-row pass of the
 * image tower on buffers of its own, for any number of prompt sets per frozen image pass (no frozen row reads a prompt,
 * trainers/rpo.py:154-156, so K / V of the frozen rows depend on the image alone).
 *   q_rows, out : [sets * B * Kp, ldq / ldo] act dtype, set-major: row (s * B + b) * Kp + j is query j of set s for image b
 *   k, v        : the frozen rows; image b reads rows (first_image[0] + b) * N ... + N, leading dimension ldkv (3 d when
 *                 they point into the packed in-proj output of the pass just run, 2 d in a cache of its K | V columns)
 *   first_image : int32 on the DEVICE (read by the kernel: one captured graph serves every chunk of a cached set), or
 *                 NULL = 0
 * One workgroup per (image, head) stages the image's K / V once and serves the query tiles of all sets.  Scores and
 * softmax in fp32, P as in rpo_attn_readonly_fwd; per query the bits do not depend on `sets` or on the other queries of
 * the launch.  head_dim 64, N <= 288, any sets * Kp.  Columns [H * 64, ldo) of `out` are not touched. */
int rpo_attn_prompt_fwd(const void* q_rows, int64_t ldq, const void* k, const void* v, int64_t ldkv,
                        void* out, int64_t ldo, int dtype, int B, int H, int N, int Kp, int sets,
                        const int32_t* first_image, float scale, void* stream);

/* (ABI 8 addition) The backward twin of rpo_attn_prompt_fwd: the prompt queries of `sets` prompt sets that were trained on
 * ONE shared batch (rpo_amd/engine_prompt_train.py).  dq = scale * (U - delta W) given da = d(loss)/d(out), with P recomputed
 * from q and K -- nothing saved by the forward -- and no dK / dV: the keys and values belong to frozen tokens.
 *   q_rows, da, dq : [sets * B * Kp, ldq / ldda / lddq] act dtype, set-major as in rpo_attn_prompt_fwd
 *   k, v, ldkv, first_image : as in rpo_attn_prompt_fwd (first_image is read on the device; NULL = 0)
 * One workgroup per (image, head) stages the image's K / V once and serves the 32-query tiles of all sets, one wave per
 * tile walking all key tiles (no cross-wave partials; fixed summation order, no atomics).  Per query the bits do not depend
 * on `sets`, on the query's place in a tile or on the other queries of the launch.  head_dim 64, N <= 288 (above:
 * RPO_E_SHAPE, nothing launched), any sets * Kp within rpo_attn_prompt_fwd's limits.  Columns [H * 64, lddq) of `dq` are
 * not touched. */
int rpo_attn_prompt_bwd(const void* q_rows, int64_t ldq, const void* k, const void* v, int64_t ldkv,
                        const void* da, int64_t ldda, void* dq, int64_t lddq, int dtype,
                        int B, int H, int N, int Kp, int sets, const int32_t* first_image, float scale, void* stream);

/* Backward of rpo_attn_readonly_fwd for the prompt rows only: dq[B*Kp, lddq] given da[B*Kp, ldda].
 * q_rows points at the first PROMPT row of q; k, v at the first frozen row.  dK/dV are not
 * produced: keys/values belong to frozen tokens.  Kp <= 128, N <= 1025 (N > 288: the keys in chunks of 256, one pass for
 * the row statistics and one for delta and dS.K; fixed summation order, no atomics). */
int rpo_attn_readonly_bwd(const void* q_rows, int64_t ldq, const void* k, const void* v, int64_t ldkv,
                          const void* da, int64_t ldda, void* dq, int64_t lddq, int dtype,
                          int B, int H, int N, int Kp, float scale, void* stream);

/* The same with the d out-proj GEMM folded in (16-bit storage, d = H * 64 = 512, 768 or 1024, Kp <= 64): dx[B*Kp, lddx] is
 * the gradient of the out-proj OUTPUT (act dtype) and w_out_t[d, ldw] the transposed out-proj weight ([in, out], as
 * packed for the dX GEMMs); every (image, head, 32-query tile) workgroup forms its slice of da = dx . W_out itself.
 * Replaces the autograd of out_proj + SDPA (clip/model.py:186) for the prompt rows with one launch. */
int rpo_attn_readonly_bwd_proj(const void* q_rows, int64_t ldq, const void* k, const void* v, int64_t ldkv,
                               const void* dx, int64_t lddx, const void* w_out_t, int64_t ldw, void* dq, int64_t lddq,
                               int dtype, int B, int H, int N, int Kp, float scale, void* stream);

/* Text-tower attention for `rows` query rows per class against that class's cached keys /
 * values kc, vc [n_cls * Lmax, ldkv] (class c uses rows c*Lmax .. c*Lmax + len[c]).
 * causal = 0: every row reads keys [0, len[c])            (prompt rows, trainers/rpo.py:146-149:
 *             causal AND col < len_c, and prompts sit at positions >= len_c)
 * causal = 1: row t reads keys [0, min(t + 1, len[c]))     (the one-off pass over the frozen tokens)
 * len: int32 device array [n_cls].  Lmax <= 128.  len[c] >= 1 is the caller's duty: an empty class has no key to
 * normalise over and both kernels write NaN rows for it (no trainer forms one: every prompt holds SOS and EOT).
 * len[c] > Lmax reads as Lmax (both kernels clamp it; the cache has no row past Lmax).
 * Kernels: 16-bit storage, causal = 0, rows <= 64, Lmax <= 96, 16-byte aligned rows -- the training path's shapes -- run as
 * ONE WAVE per (class, head) on the matrix cores (fp32 accumulation and softmax; P and dS rounded to the storage type for
 * the second contraction, as in rpo_attn_readonly_fwd); everything else as fp32 VALU arithmetic.  Same meaning either way. */
int rpo_text_attn_fwd(const void* q, int64_t ldq, const void* kc, const void* vc, int64_t ldkv,
                      void* out, int64_t ldo, int dtype, const int32_t* len, int n_cls, int rows,
                      int Lmax, int H, int causal, float scale, void* stream);

/* dq = d(loss)/d(q) of the causal = 0 case given da = d(loss)/d(out); K and V are frozen (no dk, dv).  Replaces the autograd of
 * nn.MultiheadAttention's SDPA (clip/model.py:186, trainers/rpo.py:308) for the text tower's prompt rows. */
int rpo_text_attn_bwd(const void* q, int64_t ldq, const void* kc, const void* vc, int64_t ldkv,
                      const void* da, int64_t ldda, void* dq, int64_t lddq, int dtype,
                      const int32_t* len, int n_cls, int rows, int Lmax, int H, float scale, void* stream);

/* (ABI 8 additions) The causal = 0 forward and its backward for n_cls VIRTUAL classes on a SHARED cache of n_kv real
 * classes (n_cls a multiple of n_kv, else RPO_E_SHAPE): virtual class v has its own `rows` query rows (q / out / da / dq:
 * [n_cls * rows, ld*]) and reads len[v % n_kv] and the cache rows (v % n_kv) * Lmax ... of kc, vc [n_kv * Lmax, ldkv];
 * len: int32 [n_kv].  S prompt sets of one class set are n_cls = S * n_kv virtual classes: the cache is read, never
 * replicated (one copy is ~1.9 GB in 16-bit at 1000 classes).  Same kernels and kernel choice as the plain calls; the bits
 * are those of the plain calls on a cache and `len` replicated n_cls / n_kv times.  n_kv = n_cls is the plain call. */
int rpo_text_attn_fwd_shared(const void* q, int64_t ldq, const void* kc, const void* vc, int64_t ldkv,
                             void* out, int64_t ldo, int dtype, const int32_t* len, int n_cls, int n_kv, int rows,
                             int Lmax, int H, float scale, void* stream);
int rpo_text_attn_bwd_shared(const void* q, int64_t ldq, const void* kc, const void* vc, int64_t ldkv,
                             const void* da, int64_t ldda, void* dq, int64_t lddq, int dtype,
                             const int32_t* len, int n_cls, int n_kv, int rows, int Lmax, int H, float scale, void* stream);

/* Dense backward of the text tower's causal attention: dq, dk, dv for ALL rows of every class (q, k, v, their
 * gradients: [n_cls * Lmax, ld / ldd], class c = rows c*Lmax .. c*Lmax + len[c]; row t reads keys [0, min(t + 1, len[c]))
 * as rpo_text_attn_fwd with causal = 1), given d_out = dL/d(attention output).  Replaces autograd of
 * nn.MultiheadAttention's SDPA (clip/model.py:186) under CLIP's plain causal mask (:332-338) for the sibling trainers
 * whose learned parameters sit in front of the class name (CoOp, trainers/coop.py:117-134,258-281).  Rows >= len[c]
 * get zero gradients.  Lmax <= 80 (CLIP's context is 77). */
int rpo_text_attn_bwd_dense(const void* q, const void* k, const void* v, int64_t ld, const void* d_out, int64_t lddo,
                            void* dq, void* dk, void* dv, int64_t ldd, int dtype, const int32_t* len, int n_cls,
                            int Lmax, int H, float scale, void* stream);

/* (ABI 8 addition) The causal = 1 forward for n_img * n_cls sequences of P + S positions whose first P rows are SHARED by
 * the n_cls sequences of an image -- CoCoOp's [SOS | ctx + bias[b] | name . EOT] (trainers/cocoop.py:123-161) under the plain
 * causal mask: the P = 1 + n_ctx leading rows read only themselves, so they are the same for every class of image b and are
 * stored once.  q, k, v [rows, ld] and out [rows, ldo] are ONE contiguous row set (LayerNorm and the GEMMs run over it
 * unchanged), rows = n_img * P + n_img * n_cls * S:
 *   prefix row (b, p)    at b * P + p:                            position p of every sequence of image b
 *   suffix row (b, c, s) at n_img * P + (b * n_cls + c) * S + s:  position P + s of sequence (b, c)
 * len: int32 device array [n_cls], the class's length SOS .. EOT, shared by the images; the caller guarantees
 * len[c] >= P + 3.  Prefix row (b, p) reads prefix keys (b, 0 .. p); suffix row (b, c, s) reads the P prefix keys of image
 * b, then suffix keys (b, c, 0 .. s), nk = min(P + s + 1, len[c]) keys in all (rows past the EOT: as rpo_text_attn_fwd).
 * fp32 VALU arithmetic of rpo_text_attn_fwd's causal kernel, keys in position order: given the same q / k / v values the
 * output holds THE BITS of rpo_text_attn_fwd(causal = 1, Lmax = P + S) on the sequences gathered densely to
 * [n_img * n_cls * (P + S)] rows.  One workgroup per (image, head, 4 classes, 4 suffix rows) stages the image's prefix K / V
 * head slice once.
 * P + S <= 80 (else RPO_E_SHAPE, as a launch grid over 2^31 - 1 workgroups); k, v and the rows of ld / ldo 16-byte aligned
 * (RPO_E_ALIGN); f32, bf16 and f16 storage. */
int rpo_text_attn_fwd_prefix(const void* q, const void* k, const void* v, int64_t ld, void* out, int64_t ldo,
                             int dtype, const int32_t* len, int n_img, int n_cls, int P, int S, int H,
                             float scale, void* stream);

/* (ABI 8 addition) The backward of rpo_text_attn_fwd_prefix, for training on the shared layout (CoOp's and CoCoOp's learned
 * context IS the prefix): autograd of the causal attention over the first len[c] positions of every sequence (b, c) --
 * rpo_text_attn_bwd_dense's math, fp32 throughout -- on rpo_text_attn_fwd_prefix's rows.  q, k, v [rows, ld], d_out
 * [rows, lddo] = dL/d(attention output), dq, dk, dv [rows, ldd]; len: int32 device array [n_cls], len[c] >= P + 1.
 *   suffix row (b, c, s), P + s <  len[c]: dq, dk, dv of sequence (b, c) at position P + s
 *   suffix row (b, c, s), P + s >= len[c]: exact zeros in all three (the dX GEMM reads every row)
 *   prefix row (b, j): dq from the prefix's own P x P causal attention with the prefix rows' d_out; dk and dv = that self
 *                      part + the sum over ALL n_cls classes of what their suffix queries contribute to key j
 * so a prefix row's gradient is the sum of the gradients of its n_cls dense copies.  No atomics: workgroups write fp32
 * partials per group of classes to `workspace` (at least rpo_text_attn_bwd_prefix_workspace_floats(n_img, n_cls, P, H)
 * floats, no initialisation needed), a second launch adds them in ascending group order, then the self part, and rounds
 * once.  The same bits on every call, and image b's bits are those of a launch over image b alone.
 * P + S <= 80 (else RPO_E_SHAPE, as a launch grid over 2^31 - 1 workgroups); k, v, workspace and the rows of ld / lddo / ldd
 * 16-byte aligned (RPO_E_ALIGN); f32, bf16 and f16 storage.  A refused call launches nothing. */
int rpo_text_attn_bwd_prefix(const void* q, const void* k, const void* v, int64_t ld, const void* d_out, int64_t lddo,
                             void* dq, void* dk, void* dv, int64_t ldd, int dtype, const int32_t* len, int n_img,
                             int n_cls, int P, int S, int H, float scale, float* workspace, void* stream);
/* (ABI 8 addition) fp32 elements of rpo_text_attn_bwd_prefix's workspace; 0 for non-positive arguments. */
int64_t rpo_text_attn_bwd_prefix_workspace_floats(int n_img, int n_cls, int P, int H);

/* CoCoOp's meta-net (trainers/cocoop.py:93-97, PromptLearner.forward :137-143): bias[b] = linear2(relu(linear1(f[b] /
 * |f[b]|))) for the B raw image features img_f [B, e]; w1 [h, e], b1 [h], w2 [d, h], b2 [d], all fp32.  f_norm [B, e] and
 * hidden [B, h] are kept for rpo_metanet_bwd, which turns d_bias [B, d] into the gradients of the four tensors (batch sum
 * in fixed order).  (e + h) * 4 and B * h * 4 bytes must fit 48 KB of LDS. */
int rpo_metanet_fwd(const float* img_f, const float* w1, const float* b1, const float* w2, const float* b2,
                    float* f_norm, float* hidden, float* bias, int B, int e, int h, int d, void* stream);
int rpo_metanet_bwd(const float* d_bias, const float* f_norm, const float* hidden, const float* w2,
                    float* g_w1, float* g_b1, float* g_w2, float* g_b2, int B, int e, int h, int d, void* stream);

/* Cosine-logit head, cross-entropy and their backward (trainers/rpo.py:215-230):
 *   logits[b,c] = (scale_exp / K) * sum_i <img_f[b,i]/|.|, text_f[c,i]/|.|>
 *   loss = mean_b CE(logits[b], label[b])
 * img_f [B,K,e], text_f [C,K,e], logits [B,C], loss [1], d_img_f / d_text_f like the inputs, all fp32.
 * label: int64 device array [B], or NULL for eval (only logits are written).  A target outside [0, C) makes the loss
 * NaN (F.cross_entropy raises; a kernel cannot) and reads nothing out of bounds.
 * workspace: fp32, at least rpo_head_workspace_floats(B, C, K, e) elements; no initialisation needed.
 * Two launches per training step for class sets up to 128 (logits + norms over B*C blocks; backward with the softmax
 * recomputed per block).  Above 128 classes (e a multiple of 32, 16-byte aligned features) the K pairings run as K small
 * GEMMs on the fp32 matrix pipe, six launches, every feature element read once; their scratch lies inside the same
 * workspace.  Fixed summation orders in both; e <= 1024. */
int64_t rpo_head_workspace_floats(int B, int C, int K, int e);
int rpo_head_fwd_bwd(const float* img_f, const float* text_f, const int64_t* label, float scale_exp,
                     float* logits, float* loss, float* d_img_f, float* d_text_f,
                     int B, int C, int K, int e, float* workspace, void* stream);
/* The same, also leaving act-dtype copies (RPO_BF16 / RPO_F16, round to nearest even) of the two feature gradients for
 * the dX GEMMs of the projections that follow (either may be NULL). */
int rpo_head_fwd_bwd_act(const float* img_f, const float* text_f, const int64_t* label, float scale_exp,
                         float* logits, float* loss, float* d_img_f, float* d_text_f, void* d_img_f_act,
                         void* d_text_f_act, int act_dtype, int B, int C, int K, int e, float* workspace, void* stream);

/* (ABI 8 additions) S independent heads in the launches of one (the group is a grid dimension: the launch count does not
 * grow with S): img_f [S*B, K, e], text_f [S*C, K, e], label [S*B] (or NULL: eval, logits only), logits [S*B, C], loss [S],
 * gradients like the inputs.  Group s pairs images [s B, (s+1) B) with text features [s C, (s+1) C) ONLY; loss[s] is the
 * mean over its own B images, and an out-of-range target poisons the loss and gradients of its own group alone.  Both
 * class-count regimes of rpo_head_fwd_bwd (chosen from B, C, e as there).  Per group the bits of rpo_head_fwd_bwd[_act]
 * on the group's slices.  workspace: at least S * rpo_head_workspace_floats(B, C, K, e) floats.  1 <= S <= 1024. */
int rpo_head_fwd_bwd_grouped(const float* img_f, const float* text_f, const int64_t* label, float scale_exp,
                             float* logits, float* loss, float* d_img_f, float* d_text_f,
                             int S, int B, int C, int K, int e, float* workspace, void* stream);
int rpo_head_fwd_bwd_grouped_act(const float* img_f, const float* text_f, const int64_t* label, float scale_exp,
                                 float* logits, float* loss, float* d_img_f, float* d_text_f, void* d_img_f_act,
                                 void* d_text_f_act, int act_dtype, int S, int B, int C, int K, int e, float* workspace,
                                 void* stream);

/* (ABI 8 addition) rpo_head_fwd_bwd_grouped_act with a per-group number of pairs: k_used, S int32 values on the DEVICE,
 * 1 <= k_used[s] <= K.  K is the ablated hyper-parameter of the method (configs/trainers/RPO/main_K4.yaml, main.yaml,
 * main_K24.yaml differ in it alone) and enters it in the head only (trainers/rpo.py:215-227: the mean over the K pairs);
 * group s, k = k_used[s]:
 *   logits = (scale_exp / k) * the sum over the pairs i < k;  the loss weights use scale_exp / (k B)
 *   rows i >= k of d_img_f / d_text_f and of their act copies are written as exact zeros, and rows i >= k of img_f /
 *   text_f are never read (they may hold anything, NaN included)
 * The arrays keep the stride of K rows per image / class and the workspace the layout of K; both class-count regimes, chosen
 * from B, C, e (and K) as in rpo_head_fwd_bwd_grouped; label NULL: eval, logits only.  Per group the bits of
 * rpo_head_fwd_bwd[_act] called with K = k on the compacted [B, k, e] / [C, k, e] copies of the group's first k rows.  A
 * k_used[s] outside [1, K] makes that group's logits, loss and gradients NaN (as an out-of-range target does) and reads or
 * writes nothing out of bounds.  k_used NULL: RPO_E_BADARG (callers without per-group K call the entry points above). */
int rpo_head_fwd_bwd_grouped_k(const float* img_f, const float* text_f, const int64_t* label, float scale_exp,
                               float* logits, float* loss, float* d_img_f, float* d_text_f, void* d_img_f_act,
                               void* d_text_f_act, int act_dtype, int S, int B, int C, int K, int e,
                               const int32_t* k_used, float* workspace, void* stream);

/* Linear-probe head, cross-entropy and the gradient of the probe layer (trainers/linear_prob.py:61-95, :151-184):
 *   z      = img_f . w^T + bias                 (lp_layer = nn.Linear(e, e) on the UN-normalised image feature, :89-90)
 *   logits = scale_exp * z . text_f_n^T          (text_f_n: the normalised text features of preprocess, :77-83)
 *   loss   = mean_b CE(logits[b], label[b])
 *   g_w    = dz^T . img_f,  g_bias = sum_b dz,   dz = scale_exp ((softmax - onehot) / B) . text_f_n
 * img_f [B,e], w [e,e] (out x in), bias [e], text_f_n [C,e], z [B,e], logits [B,C], loss [1], g_w [e,e], g_bias [e]; all
 * fp32, row-major; img_f, w, z, text_f_n 16-byte aligned.  label: int64 device array [B], or NULL for eval (only z and
 * logits are written; loss, g_w and g_bias are not touched).  A target outside [0, C) makes the loss NaN (and that
 * image's share of the gradients) and reads nothing out of bounds.  g_bias may be g_w + e*e (one flat [W | b] gradient).
 * workspace: fp32, at least rpo_lp_head_workspace_floats(B, C, e) elements; no initialisation needed.
 * e a multiple of 32 up to 1024, 1 <= B <= 128, 1 <= C <= 32768, else RPO_E_SHAPE.  Four launches for training, two for
 * eval, all GEMM-shaped parts on the fp32 matrix pipe, fixed summation orders (the same bits on every call). */
int64_t rpo_lp_head_workspace_floats(int B, int C, int e);
int rpo_lp_head_fwd_bwd(const float* img_f, const float* w, const float* bias, const float* text_f_n,
                        const int64_t* label, float scale_exp, float* z, float* logits, float* loss,
                        float* g_w, float* g_bias, int B, int C, int e, float* workspace, void* stream);

/* (ABI 8 addition) S linear-probe heads in the launches of one (the members of a sweep, rpo_amd/lp_sweep.py): the group is
 * a grid dimension, four launches for training and two for eval whatever S is.  img_f [B,e], text_f_n [C,e] and label [B]
 * are shared by all groups; group s has its own layer, row s of params = [W_s (e x e, out x in) | b_s (e)] with a row
 * stride of set_stride floats, and writes z[s] ([S,B,e]), logits[s] ([S,B,C]), loss[s] ([S]) and row s of grads, which
 * has the layout of params ([g_w | g_bias] per row).  Floats of a row beyond e*e + e (the padding up to set_stride) are
 * never read or written, in params and in grads.  Per group, bit for bit, what rpo_lp_head_fwd_bwd gives on (img_f, W_s,
 * b_s, text_f_n, label): the tiles, the split-k, every summation order are that call's, only the addresses differ.
 * label NULL: eval, only z and logits are written.  A target outside [0, C) poisons every group (the labels are shared)
 * as it poisons the ungrouped call.  workspace: S * rpo_lp_head_workspace_floats(B, C, e) floats, group s on slice s.
 * The limits of rpo_lp_head_fwd_bwd on B, C, e, and 1 <= S <= 1024, set_stride >= e*e + e, else RPO_E_SHAPE;
 * set_stride % 4 != 0 or img_f, params, z, text_f_n off the 16-byte grid: RPO_E_ALIGN; a NULL required pointer (grads and
 * loss are required with a label): RPO_E_BADARG.  An error launches nothing.  No atomics, no allocation, capturable. */
int rpo_lp_head_fwd_bwd_grouped(const float* img_f, const float* params, int64_t set_stride, const float* text_f_n,
                                const int64_t* label, float scale_exp, float* z, float* logits, float* loss,
                                float* grads, int S, int B, int C, int e, float* workspace, void* stream);

/* (ABI 8 additions) CoCoOp for S independent runs ("members") of b images each in the launches of one (rpo_amd/coop_multi.py;
 * rpo_amd/csrc/cocoop_sets.hip).  Member s owns row s of params / grads [S, set_stride], fp32:
 *   [ctx (n_ctx * d) | w1 (h * e) | b1 (h) | w2 (d * h) | b2 (d)]
 * -- the flat buffer of a standalone run, so a row can be copied into one and back.  Floats of a row past that length (the
 * padding up to set_stride) are never read or written.  Images, and everything per image, are member-major: image i of
 * member s is row s * b + i.
 *   rpo_metanet_fwd_sets      bias[s b + i] = linear2_s(relu(linear1_s(f / |f|))) for img_f [S*b, e]; f_norm [S*b, e] and
 *                             hidden [S*b, h] are kept for the backward.  One workgroup per (member, image); per image the
 *                             bits of rpo_metanet_fwd called with member s's four tensors.
 *   rpo_cocoop_shift_sets     c_shift[s b + i, r, :] = ctx_s[r, :] + bias[s b + i, :]   (c_shift [S*b, n_ctx, d])
 *   rpo_cocoop_grad_tail_sets per member, sums in ascending i, then r, starting from their first term:
 *                               row s of grads, ctx part = (1 / b) sum_i d_shift[s b + i]          (d_shift [S*b, n_ctx, d])
 *                               d_bias[s b + i]          = (1 / b) sum_r d_shift[s b + i, r]       (d_bias [S*b, d])
 *                               loss[s]                  = (1 / b) sum_i loss_img[s b + i]
 *                             b = 1: d_shift and loss_img themselves.  Writes nothing else of grads.
 *   rpo_metanet_bwd_sets      the member is a grid dimension; per member the bits of rpo_metanet_bwd(B = b) on its slices
 *                             of d_bias / f_norm / hidden with its w2, written into row s of grads at the four offsets
 *                             (the ctx part is not touched).
 * One launch each, fixed summation orders, no atomics, no allocation, capturable in a HIP graph.  A NULL pointer or a
 * non-positive n_ctx / e / h / d: RPO_E_BADARG.  S outside 1 .. 1024, b < 1, set_stride below the floats of a row the call
 * touches (the meta-net pair: the row length; the other two: n_ctx * d), or (e + h) * 4 (forward) / b * h * 4 (backward)
 * bytes beyond 48 KB of LDS: RPO_E_SHAPE.  set_stride % 4 != 0, or params / grads off the 16-byte grid: RPO_E_ALIGN.  An
 * error launches nothing. */
int rpo_metanet_fwd_sets(const float* img_f, const float* params, int64_t set_stride, int n_ctx, float* f_norm,
                         float* hidden, float* bias, int S, int b, int e, int h, int d, void* stream);
int rpo_cocoop_shift_sets(const float* params, int64_t set_stride, const float* bias, float* c_shift, int S, int b,
                          int n_ctx, int d, void* stream);
int rpo_cocoop_grad_tail_sets(const float* d_shift, const float* loss_img, float* grads, int64_t set_stride, float* d_bias,
                              float* loss, int S, int b, int n_ctx, int d, void* stream);
int rpo_metanet_bwd_sets(const float* d_bias, const float* f_norm, const float* hidden, const float* params, float* grads,
                         int64_t set_stride, int n_ctx, int S, int b, int e, int h, int d, void* stream);

/* (ABI 8 additions) CoOp for S independent runs ("members") with their OWN number of context vectors on one dense text pass
 * (rpo_amd/coop_sweep.py; rpo_amd/csrc/coop_sets.hip).  The prompts are those of n_max placeholders; member s has
 * n_s = n_ctx_members[s] context vectors (int32 [S] on the DEVICE, 1 <= n_s <= n_max; a value outside [0, n_max] is clamped
 * into it, so nothing is read or written out of bounds), delta = n_max - n_s, and owns row s of params / grads
 * [S, set_stride], fp32: its context is the first n_s * d floats of the row.  Rows of the pass are member-major: row
 * ((s * n_cls + c) * L + p) is position p of class c of member s.
 *   rpo_coop_fill_sets      x0[(s, c, p), :] from tok [n_cls * L, d] (the token embeddings of the n_max prompts, no
 *                           positional part) and pos [L, d]:
 *                             p = 0                     tok[c, 0] + pos[0]
 *                             1 <= p <= n_s             params[s, (p - 1) * d + :] + pos[p]
 *                             p > n_s, p + delta < L    tok[c, p + delta] + pos[p]
 *                             otherwise                 pos[p]
 *                           One fp32 add per element: the host's float32 composition, bit for bit.
 *   rpo_coop_ctx_grad_sets  grads[s, r * d + j] = the sum over the classes c of dx[(s, c, 1 + r), j] for r < n_s, IN THE
 *                           ORDER of rpo_reduce_groups(groups = n_cls, rows = n_s) (one thread per element below 64 classes,
 *                           eight partial sums per element from 64 on), read from dx [S * n_cls * L, d] in place; the
 *                           entries [n_s * d, n_max * d) of the row are written as exact zeros.
 * Floats of a row past n_max * d (the padding up to set_stride) are never read or written.  One launch each, no atomics, no
 * allocation, capturable in a HIP graph.  A NULL pointer or a non-positive n_cls / L / d: RPO_E_BADARG.  S outside 1 .. 1024,
 * n_max < 1, n_max + 1 > L, set_stride < n_max * d, S * n_cls * L beyond 2^31 - 1 (and for the fill d % 4 != 0):
 * RPO_E_SHAPE.  set_stride % 4 != 0, or params / grads (for the fill also tok, pos, x0) off the 16-byte grid: RPO_E_ALIGN.
 * An error launches nothing. */
int rpo_coop_fill_sets(const float* tok, const float* pos, const float* params, int64_t set_stride,
                       const int32_t* n_ctx_members, float* x0, int S, int n_cls, int L, int n_max, int d, void* stream);
int rpo_coop_ctx_grad_sets(const float* dx, float* grads, int64_t set_stride, const int32_t* n_ctx_members, int S, int n_cls,
                           int L, int n_max, int d, void* stream);

/* (ABI 8 addition) Prompt ensembling (trainers/zsclip.py:85-96, ZeroshotCLIP2): the classifier is the normalised mean over
 * the templates of the normalised text features.  rpo_amd/csrc/ensemble.hip.
 *   accumulate: acc[c,:] = (first ? 0 : acc[c,:]) + sum_t feat[t,c,:] / ||feat[t,c,:]||_2     t = 0 .. T-1, ascending
 *   finish:     out[c,:] = m / ||m||_2,  m = acc[c,:] / T_total
 * feat: T blocks of n_cls rows, row t * template_stride_rows + c with e valid floats and leading dimension ld >= e
 * (template_stride_rows >= n_cls where T > 1); acc, out [n_cls, e] contiguous; out may alias acc; all fp32 device memory.
 * One wave owns a class row, the sum over t is sequential in fp32, no atomics: the bits repeat, and one call over T
 * templates gives the bits of a call over the first T1 (first = 1) followed by one over the rest (first = 0) -- provided
 * both take the same element map: 16-byte loads where e % 4 == 0, ld % 4 == 0 and feat / acc (finish: acc / out) are
 * 16-byte aligned, single floats otherwise.  1 <= e <= 1024, any n_cls >= 1, T >= 1, T_total >= 1; a null pointer, a size
 * out of range, ld < e or overlapping blocks: RPO_E_BADARG with nothing launched.  A zero row gives NaN, as the reference
 * does.  One launch each on `stream`, no allocation, capturable in a HIP graph. */
int rpo_text_ensemble_accumulate(const float* feat, int64_t ld, int T, int64_t template_stride_rows, int n_cls, int e,
                                 float* acc, int first, void* stream);
int rpo_text_ensemble_finish(const float* acc, int n_cls, int e, int T_total, float* out, void* stream);

/* Classification evaluator (Dassl's `Classification.process`, and `compute_accuracy` of the CoOp / LP steps), accumulating
 * on the device: pred[b] = logits[b].max()'s index as torch computes it on the CPU for fp32 -- the FIRST index of the row
 * maximum, a row holding NaN predicts its first NaN, ties (+inf included, all -inf too) take the lowest index.
 *   counts[0] += #(pred == label), counts[1] += B, cmat[label][pred] += 1 (row = true class)
 * logits [B, C] fp32 with row stride ldl >= C; label int64 [B]; counts int64 [2]; cmat int32 [C * C] or NULL; pred int32
 * [B] or NULL (overwritten, not accumulated); all device memory.  counts and cmat ACCUMULATE across calls: the caller
 * zeroes them once and reads them back once.  A label outside [0, C) counts in the total, is never correct, writes no
 * cmat cell and reads nothing out of bounds.  Integer sums only: every order gives the same bits.  1 <= B, C <= 65536,
 * else RPO_E_SHAPE; counts 8-byte aligned.  One launch on `stream`, no allocation, capturable in a HIP graph. */
int rpo_eval_accumulate(const float* logits, int64_t ldl, const int64_t* label, int B, int C, int64_t* counts,
                        int32_t* cmat, int32_t* pred, void* stream);

/* (ABI 8 addition) S classifiers over n CACHED image features in one launch, head and evaluator fused: what
 * trainers/zsclip.py:58-63, trainers/coop.py:196-208 and trainers/linear_prob.py:85-95 compute behind `encode_image`,
 * plus rpo_eval_accumulate, without the logits' round trip through memory.  rpo_amd/csrc/classify.hip.  s < S, i < n, c < C:
 *   logits[s,i,c] = a_i * r_sc * <feat[i,:], cls[s,c,:]> + bias[s,c]
 *   a_i  = scale / ||feat[i,:]||  if norm_feat else scale;     r_sc = 1 / ||cls[s,c,:]||  if norm_cls else 1
 *   pred[s,i] = the row maximum's index by rpo_eval_accumulate's rule (torch CPU fp32: NaN first, larger, lower index)
 *   counts[s,0] += #(pred == label), counts[s,1] += n, cmat[s][label][pred] += 1
 * feat [n, e] fp32 with leading dimension ldf >= e; cls [S, C, e] fp32; bias [S, C] fp32 or NULL; label int64 [n];
 * counts int64 [S, 2]; cmat int32 [S, C, C] or NULL; pred int32 [S, n] or NULL (overwritten); logits_out [S, n, C] fp32 or
 * NULL (for tests and callers that want the values: with NULL no logit reaches memory); all device memory.  Labels as in
 * rpo_eval_accumulate: counts and cmat ACCUMULATE across calls; a label outside [0, C) counts in the total, is never
 * correct and touches no cell.  The dot product runs on the fp32 matrix pipe over the whole k range in one fixed order,
 * both norms are double sums rounded once, the sums written are integers: a row's logits and prediction do not depend on
 * which other rows, how many, or which other classifiers are in the call, and the bits repeat from run to run.
 * e a multiple of 32 up to 1024, 1 <= C <= 65536, 1 <= S <= 1024, n >= 1, else RPO_E_SHAPE; feat and cls 16-byte, counts
 * 8-byte aligned, else RPO_E_ALIGN; a null feat / cls / label / counts: RPO_E_BADARG; nothing is launched on an error.
 * One launch on `stream`, no workspace, no allocation, capturable in a HIP graph. */
int rpo_features_classify(const float* feat, int64_t ldf, const float* cls, const float* bias, const int64_t* label,
                          float scale, int norm_feat, int norm_cls, int64_t* counts, int32_t* cmat, int32_t* pred,
                          float* logits_out, int n, int C, int e, int S, void* stream);

/* (ABI 8 addition) CLIP's linear-probe protocol on CACHED image features: S L2-regularised multinomial logistic
 * regressions (the members of a regularisation / few-shot sweep) over one feature matrix.  rpo_amd/csrc/logreg.hip,
 * rpo_amd/logreg.py.  Member s < S, row i < n, class c < C:
 *   z_sic = a_i <feat[i,:], W_s[c,:]> + b_s[c],   a_i = 1 / ||feat[i,:]|| if norm_feat else 1
 *           (rpo_features_classify's logits at scale = 1, norm_cls = 0, a_i formed by the same sum)
 *   J_s   = (1 / omega[s]) sum_i w_si CE(softmax(z_si.), label[i]) + (l2[s] / 2) ||W_s||_F^2
 * rpo_logreg_loss_grad_sets: loss[s] = J_s and grads row s = dJ_s / d[W_s | b_s] at params row s.  feat [n, e] fp32 with
 * leading dimension ldf >= e; label int64 [n]; weight [S, n] fp32 >= 0 or NULL (all ones); omega float64 [S]: Omega_s =
 * sum_i w_si AS THE CALLER SUMMED IT (a_i comes from the call's own first launch, Omega_s from the caller); l2 fp32 [S];
 * params and grads [S, set_stride] fp32, row s = [W_s (C x e) | b_s (C)], floats past C e + C of a row never addressed;
 * done int32 [S] or NULL: a member with done[s] != 0 is skipped (its grads row and loss[s] stay as they are); fit_bias = 0
 * writes a zero bias gradient; loss fp32 [S]; workspace fp32, rpo_logreg_workspace_floats(n, C, e, S) elements, no
 * initialisation needed; all device memory.  A row whose label lies outside [0, C) behaves as weight 0 and reads nothing
 * out of bounds.  Three launches: logits -> softmax -> residuals r_sic = (w_si / omega[s])(p_sic - [c == label[i]]) into
 * the workspace; G_s = R_s^T (a . feat) over row chunks of 1024; the chunk partials in ascending order + l2[s] W_s.  All
 * products on the fp32 matrix pipe in a fixed k order, the softmax sums and the weight in double rounded once, every
 * cross-workgroup sum through fp32 partials added in ascending order by a later launch, no float atomics: the bits repeat
 * from run to run, and member s has the bits of an S = 1 call on its slices.
 * rpo_logreg_step_sets: one iteration of accelerated gradient descent with a fixed step and gradient restart on rows
 * x, y, grads of [S, set_stride] (`count` <= set_stride valid floats each), grads = dJ_s at y:
 *   x+ = y - grads / L[s];  t <- 1 if <grads, x+ - x> > 0;  t+ = (1 + sqrt(1 + 4 t^2)) / 2;  y+ = x+ + ((t - 1) / t+)(x+ - x)
 * t, L, tol, grad_inf fp32 [S]; done, iters int32 [S].  grad_inf[s] = ||grads_s||_inf (NaN if any entry is); where it is
 * <= tol[s], done[s] = 1 and nothing else of the member is written -- the point kept is y, the one whose gradient was
 * tested -- else x, y, t are updated and iters[s] += 1.  A member with done[s] != 0 on entry is not touched.  One
 * workgroup per member, the restart product (double) and the max-norm reduced in a fixed order.
 * Limits: e a multiple of 32 up to 1024, 1 <= C <= 1024, 1 <= S <= 1024, n >= 1, S ceil(n / 1024) <= 65535, set_stride >= C e + C, else
 * RPO_E_SHAPE;
 * a null pointer (weight and done excepted) or a non-positive stride: RPO_E_BADARG; feat, params, grads, workspace not
 * 16-byte aligned, set_stride % 4 != 0 or omega not 8-byte aligned: RPO_E_ALIGN; nothing is launched on an error.
 * rpo_logreg_workspace_floats: 0 for a non-positive argument.  The calls only enqueue on `stream`, allocate nothing and
 * are capturable in a HIP graph. */
int64_t rpo_logreg_workspace_floats(int n, int C, int e, int S);
int rpo_logreg_loss_grad_sets(const float* feat, int64_t ldf, const int64_t* label, const float* weight, const double* omega,
                              const float* l2, const float* params, int64_t set_stride, const int32_t* done, int norm_feat,
                              int fit_bias, float* grads, float* loss, int n, int C, int e, int S, float* workspace,
                              void* stream);
int rpo_logreg_step_sets(float* x, float* y, const float* grads, int64_t set_stride, int64_t count, float* t, const float* L,
                         const float* tol, int32_t* done, int32_t* iters, float* grad_inf, int S, void* stream);

/* ---- CLIP ResNet image tower (clip/model.py:10-152, rpo_amd/csrc/conv.hip) ------------------------------------------
 * Activations are NHWC in the act dtype (`dtype`: RPO_F32 / RPO_BF16 / RPO_F16): row m = (b, y, x), channels contiguous.
 * Eval-mode BatchNorm is folded into weight and bias by the caller.  Every sum runs in a fixed order (same bits per call).
 *
 * rpo_conv2d_nhwc: y[B,H,W,Cout] = relu?(conv(x[B,H,W,Cin], w) + bias [+ resid]), kernel `ksize` 1 or 3 (pad 1), stride 1,
 *   as an implicit GEMM (k = (tap, channel)); w [Cout][ksize][ksize][Cin] act dtype, bias fp32 [Cout], resid (optional)
 *   [B,H,W,Cout] act dtype, added in fp32 before the single rounding.  Cin % 16 (f32) / % 32 (16-bit) == 0,
 *   Cout % 32 == 0, else RPO_E_SHAPE; x, w, y, resid 16-byte aligned (RPO_E_ALIGN).  tile_config: 0 = choose
 *   (rpo_conv2d_plan: 64x64, the fastest measured), 1 = 64x64, 2 = 128x128, 3 = 128x64 tiles (bit-identical results).  Nothing is launched on an error. */
int rpo_conv2d_plan(int B, int H, int W, int Cout);
int rpo_conv2d_nhwc(const void* x, const void* w, const float* bias, const void* resid, void* y, int dtype,
                    int B, int H, int W, int Cin, int Cout, int ksize, int relu, int tile_config, void* stream);
/* Stem conv1 (clip/model.py:101): 3x3, stride 2, pad 1 on the fp32 NCHW image [B,3,H,W] -> y [B,H/2,W/2,Cout] NHWC act
 * dtype; w [Cout][3][3][3] act dtype, bias fp32.  H, W even, Cout % 8 == 0, Cout <= 128, else RPO_E_SHAPE. */
int rpo_conv_stem(const float* image, const void* w, const float* bias, void* y, int dtype, int B, int H, int W,
                  int Cout, int relu, void* stream);
/* AvgPool2d(k) (kernel = stride = k, clip/model.py:22,35,108) on NHWC: y [B,H/k,W/k,C].  H, W multiples of k, C % 8 == 0. */
int rpo_avgpool_nhwc(const void* x, void* y, int dtype, int B, int H, int W, int C, int k, void* stream);
/* Attention-pool tokens (clip/model.py:67-69): tokens[B, HW+1, C] = [mean_p x[b,p] | x[b,0..HW)] + pos[HW+1, C] (pos fp32;
 * the mean in fp32).  C % 8 == 0, HW + 1 <= 256. */
int rpo_attnpool_tokens(const void* x, const float* pos, void* tokens, int dtype, int B, int HW, int C, void* stream);
/* The attention pool's one query (x[0], clip/model.py:70-91): out[b, h*64 + d] = softmax_j(scale q_b,h . k_j,h) . v_j,h
 * over the T = HW + 1 tokens of image b; q fp32 [B][ldq] (after the bias, before the scale), kv [B*T, 2C] act dtype
 * (k | v), out [B, C] act dtype.  C == 64 * heads, T <= 256. */
int rpo_attnpool_attn(const float* q, int64_t ldq, const void* kv, void* out, int dtype, int B, int T, int C, int heads,
                      float scale, void* stream);

/* torch.optim.SGD (dampening 0, no nesterov) on n fp32 scalars (trainers/rpo.py:274,309):
 *   g' = grad_scale * g + wd * p;  buf = first ? g' : momentum * buf + g';  p -= lr * buf
 * grad_scale = 1 / world_size after a sum all-reduce.  Elementwise: one call over the flat [S, K*d_t + K*d_v] buffers of S
 * runs that share the rate is S calls on the rows, bit for bit. */
int rpo_sgd_step(float* p, const float* g, float* buf, int64_t n, float lr, float momentum, float wd,
                 float grad_scale, int first_step, void* stream);

/* The step as torch.cuda.amp.GradScaler.step takes it (trainers/rpo.py:298-304, PREC "amp"): if any element of g is Inf or
 * NaN, nothing is updated.  found_inf: int32[2] on the device -- [0] = this step's flag, [1] += 1 per skipped step.  Here
 * gradients are fp32 and never scaled, so this skip is all that is left of the scaler.  buf must start at zero (a
 * skipped first step then needs no special case); first_step as in rpo_sgd_step.  One workgroup. */
int rpo_sgd_step_guarded(float* p, const float* g, float* buf, int64_t n, float lr, float momentum, float wd,
                         float grad_scale, int first_step, int32_t* found_inf, void* stream);

/* (ABI 8 addition) rpo_sgd_step[_guarded] for `sets` runs with their OWN optimiser settings in one launch (LR, weight decay
 * and warm-up are what one tunes per dataset: the OPTIM block of configs/trainers/RPO/main.yaml; trainers/rpo.py:274,298-309).  Set s is
 * row s of p / g / buf (rows set_stride floats apart), of which the two segments [0, seg0) and [seg0, seg0 + seg1) -- text |
 * img -- are stepped.  All tables are on the DEVICE:
 *   hyper     float [sets, 4]: (lr, momentum, weight decay, grad_scale) of the set; a new learning rate is a copy into
 *             this table, not a new kernel argument (a captured graph of the step stays valid)
 *   used      int32 [sets, 2] or NULL (all): the number of leading floats of each of the two segments that belong to the
 *             set (clamped to the segment); elements outside are neither scanned nor read for the verdict nor written
 *   found_inf int32 [sets, 2] or NULL
 * found_inf NULL: elementwise; per element of a set the bits of rpo_sgd_step with that set's four values.  Else one
 * 1024-thread workgroup per set: per set the bits and the [flag, count] semantics of rpo_sgd_step_guarded, the scan and
 * the skip being the set's own.  set_stride >= seg0 + seg1, sets <= 65535, else RPO_E_SHAPE.  One launch. */
int rpo_sgd_step_sets(float* p, const float* g, float* buf, int64_t set_stride, int sets, const float* hyper,
                      const int32_t* used, int64_t seg0, int64_t seg1, int first_step, int32_t* found_inf, void* stream);

/* (ABI 8 addition) Dassl's optimisers beyond plain SGD (`build_optimizer(..., cfg.OPTIM)`, trainers/rpo.py:274, and the
 * step at :298-309; the same pair of calls in coop.py, cocoop.py, linear_prob.py): rpo_sgd_step_sets generalised to
 * torch.optim's SGD (dampening, Nesterov), Adam, AdamW, Adam with amsgrad and RMSprop (not centered) -- single-tensor
 * rules, maximize = False.  Set s is row s of p / g and of the fp32 state rows s0 / s1 / s2 (rows set_stride floats apart);
 * the segments [0, seg0) and [seg0, seg0 + seg1) are stepped; `used` and `found_inf` mean what they mean there.
 *   s0  SGD, RMSprop: momentum_buffer;  Adam kinds: exp_avg          (must start at zero)
 *   s1  RMSprop: square_avg;            Adam kinds: exp_avg_sq       (must start at zero; SGD does not touch it)
 *   s2  AMSGRAD: max_exp_avg_sq (must start at zero); no other kind touches it
 * All tables are on the DEVICE, so a captured graph of the step stays valid across epochs, across a resume and from the
 * very first step:
 *   kind   int32 [sets]: RPO_OPT_*.  A value outside the enum cannot be seen by the host: such a set is IGNORED on the
 *          device (nothing of it is scanned, read or written, its counter stays), and so is a set with a negative counter
 *          and an AMSGRAD set when s2 is NULL.
 *   hyper  float [sets, 8]:
 *            0 lr             1 grad_scale (1 / world_size after a sum all-reduce)         2 weight decay
 *            3 SGD, RMSprop: momentum;  Adam kinds: beta1
 *            4 SGD: dampening;  Adam kinds: beta2;  RMSprop: alpha                         5 eps (unused by SGD)
 *            6 SGD: the Nesterov flag (non-zero = on);  Adam kinds: beta1 - (float)beta1, the low-order part of column 3
 *            7 the low-order part of column 4: x - (float)x for x = dampening | beta2 | alpha
 *          torch forms 1 - beta, 1 - beta^t, lr / (1 - beta1^t) and sqrt(1 - beta2^t) in doubles from the Python floats; the
 *          kernel forms them in double from (column 3 + column 6) and (column 4 + column 7), once per workgroup, and rounds
 *          each to fp32 once.  Zero low-order parts are valid (the betas are then their fp32 roundings).
 *   step   int32 [sets]: the number of updates the set has APPLIED.  Read by the kernel (0 = the first step: SGD's
 *          buf = g'; t = step + 1 feeds the bias corrections) and advanced by one per call unless the set's step is skipped
 *          or the set is ignored.  It replaces the first_step argument of rpo_sgd_step*.  No workgroup reads a counter
 *          that a workgroup of the same launch writes: the guarded form has one workgroup per set, the elementwise form
 *          only reads and a one-thread-per-set launch behind it, inside this call, advances.
 * found_inf NULL: elementwise.  Else one 1024-thread workgroup per set: when a used gradient element of the set is Inf or
 * NaN, nothing of the set changes (p, the state rows, step[s]) and found_inf[s] = [1, += 1] (GradScaler.step does not
 * call optimizer.step(): Adam's count does not advance).  Kind SGD with dampening 0 and Nesterov off gives, per element,
 * the bits of rpo_sgd_step_sets.  s0, s1 are always required; s2 must be non-NULL when needs_s2 != 0 (the caller knows
 * whether one of its sets is AMSGRAD), else RPO_E_BADARG.  set_stride >= seg0 + seg1, sets <= 65535,
 * seg0 + seg1 <= (2^31 - 1) * 256, else RPO_E_SHAPE. */
enum { RPO_OPT_SGD = 0, RPO_OPT_ADAM = 1, RPO_OPT_ADAMW = 2, RPO_OPT_AMSGRAD = 3, RPO_OPT_RMSPROP = 4 };
int rpo_optim_step_sets(float* p, const float* g, float* s0, float* s1, float* s2, int64_t set_stride, int sets,
                        const int32_t* kind, const float* hyper, int32_t* step, const int32_t* used, int64_t seg0,
                        int64_t seg1, int needs_s2, int32_t* found_inf, void* stream);

/* fp32 -> act dtype copy with leading dimensions (weight packing at load time) */
int rpo_convert(const float* src, int64_t lds, void* dst, int dst_dtype, int64_t ldd,
                int rows, int cols, void* stream);

/* Hardware probe used by the test-suite: one wave runs one MFMA on index-coded operands so the
 * fragment layouts the kernels assume can be checked on the device.  which: 0 = 32x32x16 bf16,
 * 1 = 32x32x2 f32.  a [32, kdim], b [32, kdim] fp32 host-layout inputs (device memory),
 * d [32,32] fp32 receives D[i][j] = sum_k a[i][k] * b[j][k] as the kernels' layout map decodes it. */
int rpo_probe_mfma(int which, const float* a, const float* b, float* d, void* stream);

/* ---- on-device input transforms -------------------------------------------------------
 * Replaces, for a batch of decoded uint8 RGB images of arbitrary sizes, the reference's per-sample CPU transforms
 * selected by configs/trainers/RPO/main_K24.yaml:8-13 (INTERPOLATION bicubic, PIXEL_MEAN/STD, TRANSFORMS
 * random_resized_crop + random_flip + normalize; test: resize + center crop + normalize), whose arithmetic is
 * Pillow's 8-bit bicubic resample reached through Dassl -> torchvision (both un-vendored).  Output is
 * BIT-IDENTICAL to PIL crop -> resize(BICUBIC) -> [crop window] -> [flip] -> ToTensor -> Normalize.
 *
 * One image = crop box (PIL crop), size the crop is resized to, window of the resized image that becomes the
 * size x size output (win = 0,0 and resize = size for the train transform; the center-crop offsets at test time),
 * and a flip flag.  All random decisions are made by the caller (rpo_amd/input_pipeline.py). */
typedef struct rpo_image_desc {
  int64_t src_offset;                      /* byte offset of the image in `src` (HWC uint8 RGB, rows packed) */
  int32_t width, height;                   /* source image size */
  int32_t crop_x, crop_y, crop_w, crop_h;  /* crop box, inside the image */
  int32_t resize_w, resize_h;              /* size the crop is resized to (>= size) */
  int32_t win_x, win_y;                    /* window origin in the resized image */
  int32_t flip;                            /* horizontal flip of the output */
  int32_t reserved;
} rpo_image_desc;

/* number of taps Pillow uses for in_size -> out_size (1 when the pass is skipped); kmax of a batch = max of these */
int rpo_preprocess_ksize(int in_size, int out_size);
/* bytes of caller-owned workspace for B images, output size `size`, crops of at most max_rows rows, kmax taps */
size_t rpo_preprocess_workspace_bytes(int B, int size, int max_rows, int kmax);
/* (ABI 8 addition) The descriptor validation of rpo_preprocess_batch on its own: pure host code, no HIP call, nothing
 * launched, usable on a machine without a GPU.  desc_host: B descriptors in host memory; src_bytes: size of the buffer the
 * src_offset fields index.  A null pointer or B, size, max_rows or kmax <= 0: RPO_E_BADARG.  RPO_E_SHAPE: a non-positive
 * image or crop size, a crop box that leaves the image, resize_w/h < size, a window that leaves the resized image, or an
 * image that does not lie inside [0, src_bytes).  RPO_E_WORKSPACE: rpo_preprocess_ksize of an axis > kmax, or
 * crop_h > max_rows.  Every field may hold any value of its type: no test inside forms a sum or product that overflows. */
int rpo_preprocess_check(const rpo_image_desc* desc_host, int B, int size, int max_rows, int kmax, int64_t src_bytes);
/* src: device buffer holding the B images; desc_host/desc_dev: the same B descriptors in host and device memory
 * (the host copy is validated by rpo_preprocess_check after the pointer, workspace and alignment checks, and its code is
 * returned unchanged; the device copy is what the kernels read);
 * mean3/std3: host pointers; out: fp32 [B, 3, size, size] device.  Enqueues three kernels on `stream`. */
int rpo_preprocess_batch(const uint8_t* src, int64_t src_bytes, const rpo_image_desc* desc_host,
                         const rpo_image_desc* desc_dev, int B, int size, int max_rows, int kmax,
                         const float* mean3, const float* std3, float* out, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ---- on-device JPEG decode ---------------------------------------------------------------------------------------
 * Replaces Dassl's `read_image` (un-vendored; reached from the reference's dataset classes, datasets/oxford_pets.py:65-72
 * via DatasetWrapper.__getitem__), which is Pillow's `Image.open(path).convert("RGB")`: libjpeg's baseline path with its
 * defaults -- Huffman decode, dequantise, the "islow" integer IDCT, "fancy" (triangle) chroma upsampling, 16.16 fixed-point
 * YCbCr -> RGB.  rpo_jpeg_probe accepts baseline sequential DCT (SOF0, SOF1 with 8-bit tables), 8-bit samples, 1 component
 * (gray -> R = G = B) or 3 (YCbCr) at 4:4:4 / 4:2:2 / 4:2:0, any restart interval, one interleaved scan.  For those the
 * output is BIT-IDENTICAL to Pillow's wherever the coefficient blocks are ones an encoder can produce from 8-bit samples
 * (any quantiser); for other header-valid streams it is defined and deterministic but may differ from Pillow's.
 * Everything else is refused with its own RPO_E_JPEG_* code and is the caller's to decode on the host.  The header is parsed on the host; everything from the first entropy-coded byte on runs on the device. */
typedef struct rpo_jpeg_info {
  int32_t width, height;
  int32_t components;            /* 1 or 3 */
  int32_t h_samp, v_samp;        /* luma sampling factors: 1x1 (4:4:4, gray), 2x1 (4:2:2), 2x2 (4:2:0) */
  int32_t restart_interval;      /* MCUs per restart interval, 0 = none */
  int32_t mcus_x, mcus_y;        /* MCU grid; an MCU is h_samp * v_samp luma blocks + 2 chroma blocks (gray: 1 block) */
  int32_t units;                 /* independently decodable units of the scan: restart intervals (1 without DRI) */
  int32_t reserved;
  int64_t scan_offset;           /* first entropy-coded byte, relative to the file */
  int64_t scan_bytes;            /* from there to the end of the file (the device stops at the first marker) */
  int64_t table_bytes;           /* size of the table blob rpo_jpeg_tables writes (the same for every file) */
  int64_t coef_bytes;            /* int16 coefficient blocks of this image in the workspace (128 B per block) */
} rpo_jpeg_info;

/* One image of a batch.  The caller fills file_offset / table_offset / out_offset / info; rpo_jpeg_workspace_bytes fills
 * the rest. */
typedef struct rpo_jpeg_desc {
  int64_t file_offset;           /* the file's first byte in `files` */
  int64_t file_bytes;
  int64_t table_offset;          /* this image's table blob in `files`, 16-byte aligned */
  int64_t out_offset;            /* where its packed RGB uint8 [height, width, 3] goes in `out` */
  int64_t coef_offset;           /* (filled) its coefficient blocks in the workspace */
  int32_t unit_base;             /* (filled) index of its first unit among the batch's */
  int32_t reserved;
  rpo_jpeg_info info;
} rpo_jpeg_desc;

/* Per-image status the decode leaves in `status` (0 = decoded).  The pixels of an image with a non-zero status are
 * unspecified but deterministic, and inside its own height x width x 3 bytes. */
enum {
  RPO_JPEG_OK = 0,
  RPO_JPEG_TRUNCATED = 1,   /* the scan ended (marker or end of file) before the header's block count was decoded */
  RPO_JPEG_BAD_CODE = 2,    /* a bit pattern that is no code of the Huffman table, or a DC size above 11 */
  RPO_JPEG_BAD_INDEX = 3,   /* a run that leaves the 8x8 block */
  RPO_JPEG_NO_RESTART = 4   /* fewer restart markers than the header's restart interval implies */
};

/* HOST ONLY, no GPU work: parses the markers of `file` (never reading past nbytes) and fills *info.  Returns 0, or the
 * RPO_E_JPEG_* code that names why the device does not decode this file. */
int rpo_jpeg_probe(const uint8_t* file, int64_t nbytes, rpo_jpeg_info* info);
/* HOST ONLY: writes the file's table blob (quantisation tables in natural order + derived Huffman lookup tables of the
 * scan's components, info.table_bytes bytes) to host memory `blob`; the caller uploads it next to the file. */
int rpo_jpeg_tables(const uint8_t* file, int64_t nbytes, void* blob, int64_t blob_bytes);
/* HOST ONLY: lays the batch's workspace out -- fills coef_offset / unit_base of the n descriptors -- and returns the
 * bytes of caller-owned workspace rpo_jpeg_decode_batch needs for them (0 on a bad argument). */
size_t rpo_jpeg_workspace_bytes(rpo_jpeg_desc* descs, int n);
/* files: device buffer (16-byte aligned, files_bytes bytes) holding the n files and their table blobs; desc_host / desc_dev:
 * the same n descriptors in host and device memory (the host copy is validated -> RPO_E_SHAPE / RPO_E_WORKSPACE /
 * RPO_E_ALIGN, the device copy is what the kernels read); out: device buffer of out_bytes bytes; status: int32 [n] device.
 * n <= 65535 images of mixed sizes and modes, each of at most 2^31 - 1 pixels (RPO_E_SHAPE).  Enqueues four kernels on `stream`: restart-marker scan, entropy decode (one
 * lane per unit; every loop bound from the header, every byte read checked against the file's length), dequantise + IDCT,
 * upsample + colour conversion.  Writes only each image's own height * width * 3 bytes of `out`. */
int rpo_jpeg_decode_batch(const uint8_t* files, int64_t files_bytes, const rpo_jpeg_desc* desc_host,
                          const rpo_jpeg_desc* desc_dev, int n, uint8_t* out, int64_t out_bytes, void* workspace,
                          size_t workspace_bytes, int32_t* status, void* stream);

/* ---- progressive JPEG files (SOF2, Huffman coding, 8-bit samples) ------------------------------------------------
 * The files rpo_jpeg_probe refuses with RPO_E_JPEG_PROGRESSIVE, through entry points of their own; components, sampling and
 * colour rules are rpo_jpeg_probe's.  The scan script must be consistent and complete: DC scans have Ss = Se = 0 over any
 * subset of the components, AC scans 1 <= Ss <= Se <= 63 and one component; Ah, Al <= 13; the first scan over a
 * (component, coefficient) has Ah = 0, each later one Ah = the previous Al and Al = Ah - 1; a component's AC scans follow
 * its first DC scan; at EOI (or the end of the file) every coefficient of every component has reached Al = 0; no DQT
 * follows the first SOS.  DHT and DRI between scans hold for the scans behind them.  Anything else -> RPO_E_JPEG_SCRIPT (or
 * the code that names the frame) and the host decodes the file.  Pixels: bit-identical to the baseline file of the same
 * coefficient blocks, hence to Pillow's under the same condition as above.
 * The same rpo_jpeg_info / rpo_jpeg_desc, with: units = sum over the scans of their restart intervals, restart_interval = 0
 * (DRI is per scan), reserved = number of dependency levels (1..14; a scan's level is one more than the highest level among
 * earlier scans sharing a component and a coefficient with it), scan_offset = first entropy-coded byte of the first scan,
 * table_bytes = size of THIS file's plan blob. */
/* HOST ONLY: walks every marker of `file` and the entropy-coded bytes between them, never reading past nbytes. */
int rpo_jpeg_prog_probe(const uint8_t* file, int64_t nbytes, rpo_jpeg_info* info);
/* HOST ONLY: writes the file's plan blob (info.table_bytes bytes): quantisation tables in natural order, one record per
 * scan, the Huffman lookup tables as defined at each SOS, the byte offset at which every unit starts. */
int rpo_jpeg_prog_plan(const uint8_t* file, int64_t nbytes, void* blob, int64_t blob_bytes);
/* HOST ONLY: as rpo_jpeg_workspace_bytes, for descriptors whose infos come from rpo_jpeg_prog_probe. */
size_t rpo_jpeg_prog_workspace_bytes(rpo_jpeg_desc* descs, int n);
/* As rpo_jpeg_decode_batch (same arguments, same validation of the host descriptors, same status words), table_offset
 * naming each file's plan blob.  Kernels: zero the coefficient blocks and the status words; one entropy kernel per
 * dependency level (one lane per unit: a restart interval of a scan); then the IDCT and colour kernels of the baseline path. */
int rpo_jpeg_prog_decode_batch(const uint8_t* files, int64_t files_bytes, const rpo_jpeg_desc* desc_host,
                               const rpo_jpeg_desc* desc_dev, int n, uint8_t* out, int64_t out_bytes, void* workspace,
                               size_t workspace_bytes, int32_t* status, void* stream);

/* Empirical peaks of the box, used as second denominators by bench.py.
 * rpo_probe_peak_mfma: `blocks` workgroups of 4 waves each run `iters` rounds of 4 independent 32x32 MFMAs
 * (which: 0 = 32x32x16 bf16 on non-zero operands, 1 = 32x32x2 f32, 2 = 32x32x16 bf16 on ZERO operands: the chip
 * clocks to its power budget, so 0 and 2 bracket the sustained and the datasheet rate); *flops receives the flop
 * count of the launch (time it with events).  rpo_probe_peak_copy: 16-B-per-lane grid-stride copy of `bytes` bytes. */
int rpo_probe_peak_mfma(int which, int blocks, int iters, float* sink, double* flops, void* stream);
int rpo_probe_peak_copy(const void* src, void* dst, int64_t bytes, void* stream);

#ifdef __cplusplus
}
#endif
#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

/* Measured-and-not-adopted experiments of rounds 3 / 4 (paired launches, the fused MLP launch, the persistent backward
 * chain) are NOT part of this interface: they are declared in rpo_amd_experimental.h and compiled only into the
 * -DRPO_EXPERIMENTAL build of the library (python -m rpo_amd.build --experimental). */
#ifdef RPO_EXPERIMENTAL
#include "rpo_amd_experimental.h"
#endif
#endif /* RPO_AMD_H */
