// On-device baseline JPEG decode into packed RGB.  Replaces the host decode in front of the resident image
// set: Dassl's `read_image` = Pillow's `Image.open(path).convert("RGB")` = libjpeg's baseline path with its defaults.  The
// arithmetic restated (from its published statement: ITU T.81 + the Independent JPEG Group's documented integer paths):
//   Huffman decode, FF 00 unstuffing, DC prediction, zig-zag -> natural order
//   dequantise + "islow" 8x8 IDCT: 13-bit constants, columns descaled by 11 bits, rows by 18, +128, clamp
//   "fancy" chroma upsampling: h2v1 (3a + b + 1|2) >> 2; h2v2 column sums 3 near + far, then (3t + n + 8|7) >> 4; edges
//     replicated at the downsampled size; a chroma plane at most 2 samples wide is replicated instead
//   YCbCr -> RGB in 16.16 fixed point
// All integer and all defined (sums that can leave 31 bits are formed modulo 2^32), so the result depends on neither the
// launch geometry nor the batch.  Bit-identical to Pillow's for coefficient blocks an encoder can produce from 8-bit
// samples, at any quantiser; for other header-valid streams it is what tests/jpeg_oracle.py computes and may differ from
// Pillow (tests/test_gpu_jpeg.py, tests/test_jpeg_streams_host.py).
//
// The header is parsed on the host (parse_header below; plain C++, never reads past nbytes).  Four kernels per batch:
//   restart_scan_kernel  per image: status = 0; byte offsets of the RSTn markers -> workspace (unit u starts behind marker u-1)
//   entropy_kernel       one LANE per unit (image, or restart interval where DRI is present): sequential Huffman decode
//                        into int16 coefficient blocks (128 B each, MCU order) in the workspace; up to 4096 units run one
//                        per wave with the image's tables in LDS
//   idct_kernel          one lane per block: dequantise + IDCT; the 64 uint8 samples overwrite the block's first 64 bytes
//   colour_kernel        one lane per output pixel: sample fetch, upsample, colour conversion, 3 byte stores
// What bounds the entropy kernel -- the only one that reads untrusted bytes: the block count, <= 63 AC iterations per block
// (k strictly increases), <= 16 code lengths and <= 8 bytes per refill are all header / compile-time bounds; every byte read
// goes through Bits::byte_at, which checks [begin, end) of the file; every table-derived index is masked.  A corrupt stream
// therefore ends in a per-image status word and zeroed remaining blocks, never in a long or out-of-bounds run.
// Progressive (SOF2) files take entry points of their own -- rpo_jpeg_prog_* -- in the second half of this file: a host walk
// of all scans, one entropy kernel per dependency level of the scan script, then idct_kernel and colour_kernel as they are.
#include "common.h"

#include <stddef.h>
#include <string.h>

#include <algorithm>
#include <vector>

namespace {

#define HD __host__ __device__ __forceinline__
// the coefficient workspace is written as int16 and as 4 / 16-byte words, the files are read as bytes and 8-byte words
typedef uint32_t __attribute__((may_alias)) u32a_t;
typedef uint64_t __attribute__((may_alias)) u64a_t;
typedef int4 __attribute__((may_alias)) int4a_t;
typedef int16_t __attribute__((may_alias)) i16a_t;

struct HuffTab {
  uint16_t look[512];     // 9-bit lookahead: (length << 8) | symbol, 0 = the code is longer than 9 bits
  int32_t maxcode[18];    // [l] = largest code of length l, -1 = none
  int32_t valoff[18];     // [l] = index of the first value of length l minus its code
  uint8_t vals[256];
};
struct Tables {           // the per-image blob rpo_jpeg_tables writes: indexed by component of the scan
  uint16_t quant[3][64];  // natural order
  HuffTab dc[3], ac[3];
};
static_assert(sizeof(HuffTab) == 1424 && sizeof(Tables) == 384 + 6 * 1424 && sizeof(Tables) % 16 == 0, "blob layout");
static_assert(sizeof(rpo_jpeg_info) == 72 && sizeof(rpo_jpeg_desc) == 120, "descriptor layout");

__device__ __constant__ uint8_t ZIGZAG_D[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48,
    41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38,
    31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
const uint8_t ZIGZAG_H[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48,
    41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38,
    31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

HD int zigzag(int k) {
#ifdef __HIP_DEVICE_COMPILE__
  return ZIGZAG_D[k & 63];
#else
  return ZIGZAG_H[k & 63];
#endif
}

HD int blocks_per_mcu(const rpo_jpeg_info& f) { return f.components == 1 ? 1 : f.h_samp * f.v_samp + 2; }

// ---- the entropy-coded segment as a bit source ------------------------------------------------------------------
// Bytes come from `base` in aligned 8-byte words; a word is loaded whole only if it lies inside [0, total) of the buffer,
// and only bytes of [pos, end) -- this file's scan -- are ever USED.  At a marker (FF followed by anything but 00) or at
// `end` the source feeds zero bytes and counts them: a decode that consumed one of those bits overran the data.
struct Bits {
  const uint8_t* base;
  int64_t pos, end, total;
  int64_t word_idx;
  uint64_t word, next_word;
  uint64_t buf;
  int nbits, fake;

  HD void init(const uint8_t* b, int64_t p, int64_t e, int64_t t) {
    base = b; pos = p; end = e; total = t; word_idx = -2; word = 0; next_word = 0; buf = 0; nbits = 0; fake = 0;
  }
  HD uint64_t load_word(int64_t wi) const {   // bytes [8 wi, 8 wi + 8) of the buffer, zero beyond `total`
    if (wi * 8 + 8 <= total) return *reinterpret_cast<const u64a_t*>(base + wi * 8);
    uint64_t w = 0;
    for (int i = 0; i < 8; ++i)
      if (wi * 8 + i < total) w |= (uint64_t)base[wi * 8 + i] << (8 * i);
    return w;
  }
  HD uint32_t byte_at(int64_t p) {           // p in [0, total) by the caller's pos < end <= total
    const int64_t wi = p >> 3;
    if (wi != word_idx) {                    // the stream advances word by word: the following word is requested now and
      word = wi == word_idx + 1 ? next_word : load_word(wi);   // used at the next switch, its latency behind the decode
      word_idx = wi;
      next_word = load_word(wi + 1);
    }
    return (uint32_t)(word >> ((p & 7) * 8)) & 255u;
  }
  HD void refill() {                         // at most 8 iterations: nbits grows by 8 each
    while (nbits <= 56) {
      uint32_t b = 0;
      if (fake == 0 && pos < end) {
        b = byte_at(pos);
        if (b == 0xFFu) {
          const uint32_t b2 = pos + 1 < end ? byte_at(pos + 1) : 0xD9u;
          if (b2 == 0) pos += 2;
          else { b = 0; fake = 8; }
        } else {
          ++pos;
        }
      } else {
        fake += 8;
      }
      buf |= (uint64_t)b << (56 - nbits);
      nbits += 8;
    }
  }
  HD uint32_t peek(int n) const { return (uint32_t)(buf >> (64 - n)); }      // 1 <= n <= 32
  HD void skip(int n) { buf <<= n; nbits -= n; }
  HD bool overrun() const { return fake > nbits; }
};

// One Huffman symbol; needs >= 16 bits in the buffer.  Returns -1 for a pattern that is no code.
HD int huff_symbol(Bits& br, const HuffTab* t) {
  const uint32_t e = t->look[br.peek(9)];
  if (e) {
    br.skip((int)(e >> 8) & 15);
    return (int)(e & 255u);
  }
  const int32_t code16 = (int32_t)br.peek(16);
  for (int l = 10; l <= 16; ++l) {
    const int32_t code = code16 >> (16 - l);
    if (code <= t->maxcode[l]) {
      br.skip(l);
      return t->vals[(code + t->valoff[l]) & 255];
    }
  }
  return -1;
}

HD int extend(uint32_t v, int s) { return (int)v < (1 << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }

HD void zero_block(i16a_t* blk) {
  int4a_t* p = reinterpret_cast<int4a_t*>(blk);
  for (int i = 0; i < 8; ++i) p[i] = int4{0, 0, 0, 0};
}

// Unit `unit` of image d: MCUs [unit * ri, +ri) (all of them without DRI), starting `start` bytes into the scan (< 0: its
// restart marker was not found).  Returns the RPO_JPEG_* status.  Blocks behind an error are left zero.
HD int decode_unit(const uint8_t* files, int64_t files_bytes, const rpo_jpeg_desc& d, const Tables* tab, int16_t* coef,
                   int unit, int start) {
  const rpo_jpeg_info& f = d.info;
  const int total = f.mcus_x * f.mcus_y;
  const int ri = f.restart_interval > 0 ? f.restart_interval : total;
  const int mcu0 = unit * ri;
  const int nmcu = min(ri, total - mcu0);
  const int bpm = blocks_per_mcu(f), luma = bpm == 1 ? 1 : bpm - 2;
  int err = start < 0 ? RPO_JPEG_NO_RESTART : RPO_JPEG_OK;
  const int64_t scan0 = d.file_offset + f.scan_offset;
  Bits br;
  br.init(files, scan0 + (start < 0 ? 0 : start), scan0 + f.scan_bytes, files_bytes);
  if (start < 0 || start > f.scan_bytes) br.pos = br.end;
  uint32_t pred[3] = {0, 0, 0};            // modulo 2^32: the block keeps its low 16 bits, as a JCOEF does
  for (int m = 0; m < nmcu; ++m) {
    for (int j = 0; j < bpm; ++j) {
      i16a_t* blk = coef + ((int64_t)(mcu0 + m) * bpm + j) * 64;
      zero_block(blk);
      if (err) continue;
      const int c = j < luma ? 0 : j - luma + 1;
      br.refill();
      int s = huff_symbol(br, &tab->dc[c]);
      if (s < 0 || s > 11) { err = RPO_JPEG_BAD_CODE; continue; }
      if (s) {
        pred[c] += (uint32_t)extend(br.peek(s), s);
        br.skip(s);
      }
      blk[0] = (int16_t)(uint16_t)pred[c];
      for (int k = 1; k < 64;) {             // k grows by >= 1 per iteration
        br.refill();
        const int rs = huff_symbol(br, &tab->ac[c]);
        if (rs < 0) { err = RPO_JPEG_BAD_CODE; break; }
        const int r = rs >> 4;
        s = rs & 15;
        if (s) {
          k += r;
          if (k > 63) { err = RPO_JPEG_BAD_INDEX; break; }
          blk[zigzag(k)] = (int16_t)extend(br.peek(s), s);
          br.skip(s);
          ++k;
        } else if (r == 15) {
          k += 16;
        } else {
          break;
        }
      }
      if (!err && br.overrun()) err = RPO_JPEG_TRUNCATED;
    }
  }
  return err;
}

// ---- dequantise + IDCT ------------------------------------------------------------------------------------------
// The butterflies run in uint32_t: a coefficient stream no encoder writes (int16 coefficient x quantiser up to 255, dense)
// takes the sums past 31 bits, which is undefined for int and wraps modulo 2^32 here.  Only the descaling shift reads the
// sum as a signed number, so every input that stays inside 31 bits -- all an encoder produces from 8-bit samples -- gives
// the bits it gave before, at the same instruction count (tests/jpeg_oracle.py restates the same definition).
HD int descale(uint32_t v, int shift) { return (int)(v + (1u << (shift - 1))) >> shift; }

HD void idct_1d(const int* in, int stride, int* out, int ostride, int shift) {
  typedef uint32_t u;
  const u in0 = (u)in[0], in1 = (u)in[stride], in2 = (u)in[2 * stride], in3 = (u)in[3 * stride], in4 = (u)in[4 * stride],
          in5 = (u)in[5 * stride], in6 = (u)in[6 * stride], in7 = (u)in[7 * stride];
  u z1 = (in2 + in6) * 4433u;
  const u tmp2 = z1 - in6 * 15137u, tmp3 = z1 + in2 * 6270u;
  const u tmp0 = (in0 + in4) * 8192u, tmp1 = (in0 - in4) * 8192u;
  const u tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  u t0 = in7, t1 = in5, t2 = in3, t3 = in1;
  z1 = t0 + t3;
  u z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
  const u z5 = (z3 + z4) * 9633u;
  t0 *= 2446u; t1 *= 16819u; t2 *= 25172u; t3 *= 12299u;
  z1 = 0u - z1 * 7373u; z2 = 0u - z2 * 20995u;
  z3 = z5 - z3 * 16069u;
  z4 = z5 - z4 * 3196u;
  t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
  out[0] = descale(tmp10 + t3, shift);
  out[7 * ostride] = descale(tmp10 - t3, shift);
  out[ostride] = descale(tmp11 + t2, shift);
  out[6 * ostride] = descale(tmp11 - t2, shift);
  out[2 * ostride] = descale(tmp12 + t1, shift);
  out[5 * ostride] = descale(tmp12 - t1, shift);
  out[3 * ostride] = descale(tmp13 + t0, shift);
  out[4 * ostride] = descale(tmp13 - t0, shift);
}

// blk: 64 int16 coefficients in natural order -> 64 uint8 samples (row-major) over its first 64 bytes
HD void idct_block(i16a_t* blk, const uint16_t* q) {
  int v[64], w[64];
#pragma unroll
  for (int i = 0; i < 64; ++i) v[i] = (int)blk[i] * (int)q[i];
#pragma unroll
  for (int c = 0; c < 8; ++c) idct_1d(v + c, 8, w + c, 8, 11);       // columns
  uint8_t* o = reinterpret_cast<uint8_t*>(blk);
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    int row[8];
    idct_1d(w + 8 * r, 1, row, 1, 18);                               // rows
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      lo |= (uint32_t)min(max(row[i] + 128, 0), 255) << (8 * i);
      hi |= (uint32_t)min(max(row[i + 4] + 128, 0), 255) << (8 * i);
    }
    reinterpret_cast<u32a_t*>(o)[2 * r] = lo;
    reinterpret_cast<u32a_t*>(o)[2 * r + 1] = hi;
  }
}

// ---- upsample + colour conversion -------------------------------------------------------------------------------
// sample (x, y) of component c; blocks are in MCU order, 128 bytes apart, samples in the first 64
HD int sample_at(const uint8_t* coef, const rpo_jpeg_info& f, int c, int x, int y) {
  const int bx = x >> 3, by = y >> 3;
  int64_t blk;
  if (f.components == 1) {
    blk = (int64_t)by * f.mcus_x + bx;
  } else {
    const int hv = f.h_samp * f.v_samp;
    if (c == 0)
      blk = ((int64_t)(by / f.v_samp) * f.mcus_x + bx / f.h_samp) * (hv + 2) + (by % f.v_samp) * f.h_samp + bx % f.h_samp;
    else
      blk = ((int64_t)by * f.mcus_x + bx) * (hv + 2) + hv + c - 1;
  }
  return coef[blk * 128 + (y & 7) * 8 + (x & 7)];
}

HD int chroma_at(const uint8_t* coef, const rpo_jpeg_info& f, int c, int x, int y) {
  if (f.h_samp == 1) return sample_at(coef, f, c, x, y);
  const int cw = (f.width + 1) >> 1;
  if (cw <= 2) return sample_at(coef, f, c, x >> 1, f.v_samp == 2 ? y >> 1 : y);
  const int cx = x >> 1, odd = x & 1;
  const int nx = odd ? min(cx + 1, cw - 1) : max(cx - 1, 0);
  if (f.v_samp == 1)
    return (3 * sample_at(coef, f, c, cx, y) + sample_at(coef, f, c, nx, y) + 1 + odd) >> 2;
  const int ch = (f.height + 1) >> 1;
  const int cy = y >> 1, fy = (y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);
  const int t = 3 * sample_at(coef, f, c, cx, cy) + sample_at(coef, f, c, cx, fy);
  const int n = 3 * sample_at(coef, f, c, nx, cy) + sample_at(coef, f, c, nx, fy);
  return (3 * t + n + 8 - odd) >> 4;
}

HD void pixel_rgb(const uint8_t* coef, const rpo_jpeg_info& f, int x, int y, uint8_t* out) {
  const int Y = sample_at(coef, f, 0, x, y);
  if (f.components == 1) {
    out[0] = out[1] = out[2] = (uint8_t)Y;
    return;
  }
  const int cb = chroma_at(coef, f, 1, x, y) - 128, cr = chroma_at(coef, f, 2, x, y) - 128;
  const int r = Y + ((91881 * cr + 32768) >> 16);
  const int g = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16);
  const int b = Y + ((116130 * cb + 32768) >> 16);
  out[0] = (uint8_t)min(max(r, 0), 255);
  out[1] = (uint8_t)min(max(g, 0), 255);
  out[2] = (uint8_t)min(max(b, 0), 255);
}

// ---- kernels ----------------------------------------------------------------------------------------------------
constexpr int SCAN_THREADS = 256;

HD bool rst_at(const uint8_t* p, int64_t i) { return p[i] == 0xFF && (p[i + 1] & 0xF8) == 0xD0; }   // needs i + 1 < n

__global__ __launch_bounds__(SCAN_THREADS) void restart_scan_kernel(const uint8_t* __restrict__ files,
                                                                    const rpo_jpeg_desc* __restrict__ desc, int32_t* rst,
                                                                    int32_t* status) {
  __shared__ int counts[SCAN_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const rpo_jpeg_desc d = desc[b];
  const int units = d.info.units;
  int32_t* mine = rst + d.unit_base;
  if (tid == 0) status[b] = RPO_JPEG_OK;
  for (int u = tid; u < units; u += SCAN_THREADS) mine[u] = u == 0 ? 0 : -1;
  if (units <= 1) return;                                  // uniform per block
  __syncthreads();
  const uint8_t* p = files + d.file_offset + d.info.scan_offset;
  const int64_t n = d.info.scan_bytes;                     // pairs (i, i + 1) with i + 1 < n
  const int64_t chunk = (n + SCAN_THREADS - 1) / SCAN_THREADS;
  const int64_t lo = tid * chunk, hi = min(lo + chunk, n - 1);
  int cnt = 0;
  for (int64_t i = lo; i < hi; ++i) cnt += rst_at(p, i);
  counts[tid] = cnt;
  __syncthreads();
  for (int off = 1; off < SCAN_THREADS; off <<= 1) {       // inclusive scan
    const int v = tid >= off ? counts[tid - off] : 0;
    __syncthreads();
    counts[tid] += v;
    __syncthreads();
  }
  int ord = counts[tid] - cnt;                             // markers before this thread's chunk
  for (int64_t i = lo; i < hi; ++i) {
    if (rst_at(p, i)) {
      if (ord + 1 < units) mine[ord + 1] = (int32_t)(i + 2);
      ++ord;
    }
  }
}

// `lanes` active lanes per 64-lane block.  Few units (<= 4096, the usual case: one per image) -> ONE_PER_BLOCK: one unit per
// wave, no divergence, and the wave first copies its image's table blob into LDS, so the table look-up on the decode's
// dependency chain is an LDS read instead of a global one.  More units -> up to 64 per wave, tables read from global memory.
template <bool ONE_PER_BLOCK>
__global__ __launch_bounds__(64) void entropy_kernel(const uint8_t* __restrict__ files, int64_t files_bytes,
                                                     const rpo_jpeg_desc* __restrict__ desc, int n, int total_units, int lanes,
                                                     char* ws, int32_t* status) {
  __shared__ int4 lds_tab[ONE_PER_BLOCK ? sizeof(Tables) / 16 : 1];
  if (!ONE_PER_BLOCK && (int)threadIdx.x >= lanes) return;
  const int u = ONE_PER_BLOCK ? (int)blockIdx.x : blockIdx.x * lanes + threadIdx.x;
  if (u >= total_units) return;                            // block-uniform when ONE_PER_BLOCK
  int lo = 0, hi = n - 1;                                  // last image with unit_base <= u; <= 16 steps (n <= 65535)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (desc[mid].unit_base <= u) lo = mid; else hi = mid - 1;
  }
  const rpo_jpeg_desc d = desc[lo];
  const int unit = u - d.unit_base;
  const Tables* tab = reinterpret_cast<const Tables*>(files + d.table_offset);
  if (ONE_PER_BLOCK) {
    const int4* src = reinterpret_cast<const int4*>(tab);
    for (int i = threadIdx.x; i < (int)(sizeof(Tables) / 16); i += 64) lds_tab[i] = src[i];
    __syncthreads();
    if (threadIdx.x != 0) return;
    tab = reinterpret_cast<const Tables*>(lds_tab);
  }
  if (unit >= d.info.units) return;
  const int32_t* rst = reinterpret_cast<const int32_t*>(ws);
  const int err = decode_unit(files, files_bytes, d, tab, reinterpret_cast<int16_t*>(ws + d.coef_offset), unit, rst[u]);
  if (err) atomicMax(status + lo, err);
}

__global__ __launch_bounds__(256) void idct_kernel(const uint8_t* __restrict__ files, const rpo_jpeg_desc* __restrict__ desc,
                                                   char* ws) {
  const int b = blockIdx.y;
  const rpo_jpeg_desc d = desc[b];
  const int bpm = blocks_per_mcu(d.info), luma = bpm == 1 ? 1 : bpm - 2;
  const int nblk = d.info.mcus_x * d.info.mcus_y * bpm;
  const Tables* tab = reinterpret_cast<const Tables*>(files + d.table_offset);
  int16_t* coef = reinterpret_cast<int16_t*>(ws + d.coef_offset);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nblk; i += gridDim.x * blockDim.x) {
    const int j = i % bpm;
    idct_block(coef + (int64_t)i * 64, tab->quant[j < luma ? 0 : j - luma + 1]);
  }
}

__global__ __launch_bounds__(256) void colour_kernel(const rpo_jpeg_desc* __restrict__ desc, const char* ws, uint8_t* out) {
  const int b = blockIdx.y;
  const rpo_jpeg_desc d = desc[b];
  const uint8_t* coef = reinterpret_cast<const uint8_t*>(ws + d.coef_offset);
  uint8_t* o = out + d.out_offset;
  const int W = d.info.width, npix = W * d.info.height;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += gridDim.x * blockDim.x) {
    uint8_t rgb[3];
    pixel_rgb(coef, d.info, i % W, i / W, rgb);
    o[(int64_t)i * 3] = rgb[0]; o[(int64_t)i * 3 + 1] = rgb[1]; o[(int64_t)i * 3 + 2] = rgb[2];
  }
}

// ---- host: header parsing ---------------------------------------------------------------------------------------
struct RawHuff { bool set; uint8_t bits[17]; uint8_t vals[256]; int count; };
struct Parsed {
  rpo_jpeg_info info;
  uint8_t qtab[4][64];      // zig-zag order, as in the file
  bool qset[4];
  RawHuff huff[2][4];
  int comp_q[3], comp_dc[3], comp_ac[3];
};

// one DQT / DHT segment into P (shared by the baseline and the progressive header walk)
int parse_dqt(const uint8_t* seg, int sl, Parsed& P) {
  for (int q = 0; q < sl;) {
    const int pq = seg[q] >> 4, tq = seg[q] & 15;
    if (tq > 3) return RPO_E_JPEG_CORRUPT;
    if (pq) return RPO_E_JPEG_PRECISION;
    if (q + 65 > sl) return RPO_E_JPEG_CORRUPT;
    memcpy(P.qtab[tq], seg + q + 1, 64);
    P.qset[tq] = true;
    q += 65;
  }
  return 0;
}

int parse_dht(const uint8_t* seg, int sl, Parsed& P) {
  for (int q = 0; q < sl;) {
    if (q + 17 > sl) return RPO_E_JPEG_CORRUPT;
    const int tc = seg[q] >> 4, th = seg[q] & 15;
    if (tc > 1 || th > 3) return RPO_E_JPEG_CORRUPT;
    RawHuff& h = P.huff[tc][th];
    int cnt = 0;
    h.bits[0] = 0;
    for (int i = 1; i <= 16; ++i) { h.bits[i] = seg[q + i]; cnt += h.bits[i]; }
    if (cnt > 256 || q + 17 + cnt > sl) return RPO_E_JPEG_CORRUPT;
    int code = 0;                                       // the lengths must describe a prefix code
    for (int l = 1; l <= 16; ++l) {
      code += h.bits[l];
      if (code > (1 << l)) return RPO_E_JPEG_CORRUPT;
      code <<= 1;
    }
    memcpy(h.vals, seg + q + 17, cnt);
    h.count = cnt;
    h.set = true;
    q += 17 + cnt;
  }
  return 0;
}

int parse_header(const uint8_t* p, int64_t n, Parsed& P) {
  memset(&P, 0, sizeof(P));
  if (n < 4 || p[0] != 0xFF || p[1] != 0xD8) return RPO_E_JPEG_CORRUPT;
  int64_t pos = 2;
  bool have_frame = false, jfif = false;
  int adobe = -1, nc = 0;
  uint8_t cid[4] = {0}, ch[4] = {0}, cv[4] = {0}, cq[4] = {0};
  for (;;) {
    if (pos + 2 > n || p[pos] != 0xFF) return RPO_E_JPEG_CORRUPT;
    const int m = p[pos + 1];
    pos += 2;
    if (m == 0xFF) { pos -= 1; continue; }                 // fill byte
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;   // standalone markers
    if (m == 0xD9 || m == 0xD8) return RPO_E_JPEG_CORRUPT;
    if (pos + 2 > n) return RPO_E_JPEG_CORRUPT;
    const int L = (p[pos] << 8) | p[pos + 1];
    if (L < 2 || pos + L > n) return RPO_E_JPEG_CORRUPT;
    const uint8_t* seg = p + pos + 2;
    const int sl = L - 2;
    pos += L;
    if (m == 0xC2 || m == 0xC6 || m == 0xCA || m == 0xCE) return RPO_E_JPEG_PROGRESSIVE;
    if (m == 0xC9 || m == 0xCB || m == 0xCD || m == 0xCF || m == 0xCC) return RPO_E_JPEG_ARITHMETIC;
    if (m == 0xC3 || m == 0xC5 || m == 0xC7) return RPO_E_JPEG_LOSSLESS;
    if (m == 0xC0 || m == 0xC1) {
      if (have_frame || sl < 6) return RPO_E_JPEG_CORRUPT;
      if (seg[0] != 8) return RPO_E_JPEG_PRECISION;
      P.info.height = (seg[1] << 8) | seg[2];
      P.info.width = (seg[3] << 8) | seg[4];
      nc = seg[5];
      if (sl != 6 + 3 * nc || P.info.height == 0 || P.info.width == 0) return RPO_E_JPEG_CORRUPT;
      if (nc != 1 && nc != 3) return RPO_E_JPEG_COMPONENTS;
      for (int i = 0; i < nc; ++i) {
        cid[i] = seg[6 + 3 * i]; ch[i] = seg[7 + 3 * i] >> 4; cv[i] = seg[7 + 3 * i] & 15; cq[i] = seg[8 + 3 * i];
        if (cq[i] > 3 || ch[i] == 0 || cv[i] == 0) return RPO_E_JPEG_CORRUPT;
      }
      P.info.components = nc;
      have_frame = true;
    } else if (m == 0xDB) {
      const int rc = parse_dqt(seg, sl, P);
      if (rc) return rc;
    } else if (m == 0xC4) {
      const int rc = parse_dht(seg, sl, P);
      if (rc) return rc;
    } else if (m == 0xDD) {
      if (sl != 2) return RPO_E_JPEG_CORRUPT;
      P.info.restart_interval = (seg[0] << 8) | seg[1];
    } else if (m == 0xE0) {
      if (sl >= 5 && memcmp(seg, "JFIF\0", 5) == 0) jfif = true;
    } else if (m == 0xEE) {
      if (sl >= 12 && memcmp(seg, "Adobe", 5) == 0) adobe = seg[11];
    } else if (m == 0xDA) {
      if (!have_frame) return RPO_E_JPEG_CORRUPT;
      const int ns = sl > 0 ? seg[0] : 0;
      if (sl != 4 + 2 * ns) return RPO_E_JPEG_CORRUPT;
      if (ns != nc) return RPO_E_JPEG_MULTISCAN;
      P.info.h_samp = P.info.v_samp = 1;
      if (nc == 3) {
        const bool rgb_ids = cid[0] == 'R' && cid[1] == 'G' && cid[2] == 'B';
        if (!jfif && (adobe == 0 || (adobe < 0 && rgb_ids))) return RPO_E_JPEG_RGB;
        if (ch[1] != 1 || cv[1] != 1 || ch[2] != 1 || cv[2] != 1) return RPO_E_JPEG_SAMPLING;
        if (!((ch[0] == 1 && cv[0] == 1) || (ch[0] == 2 && cv[0] == 1) || (ch[0] == 2 && cv[0] == 2)))
          return RPO_E_JPEG_SAMPLING;
        P.info.h_samp = ch[0];
        P.info.v_samp = cv[0];
      }
      for (int i = 0; i < ns; ++i) {
        if (seg[1 + 2 * i] != cid[i]) return RPO_E_JPEG_MULTISCAN;
        const int td = seg[2 + 2 * i] >> 4, ta = seg[2 + 2 * i] & 15;
        if (td > 3 || ta > 3 || !P.qset[cq[i]] || !P.huff[0][td].set || !P.huff[1][ta].set) return RPO_E_JPEG_CORRUPT;
        P.comp_q[i] = cq[i]; P.comp_dc[i] = td; P.comp_ac[i] = ta;
      }
      rpo_jpeg_info& f = P.info;
      f.mcus_x = (f.width + 8 * f.h_samp - 1) / (8 * f.h_samp);
      f.mcus_y = (f.height + 8 * f.v_samp - 1) / (8 * f.v_samp);
      const int total = f.mcus_x * f.mcus_y;
      f.units = f.restart_interval ? (total + f.restart_interval - 1) / f.restart_interval : 1;
      f.scan_offset = pos;
      f.scan_bytes = n - pos;
      f.table_bytes = sizeof(Tables);
      f.coef_bytes = (int64_t)total * blocks_per_mcu(f) * 128;
      return 0;
    }
    // every other segment (APPn, COM, DNL, ...) is skipped
  }
}

void derive(const RawHuff& h, HuffTab& t) {
  memset(&t, 0, sizeof(t));
  memcpy(t.vals, h.vals, h.count);
  int code = 0, p = 0;
  for (int l = 1; l <= 16; ++l) {
    const int nb = h.bits[l];
    t.maxcode[l] = nb ? code + nb - 1 : -1;
    t.valoff[l] = p - code;
    if (l <= 9)
      for (int i = 0; i < nb; ++i)
        for (int k = 0; k < (1 << (9 - l)); ++k)
          t.look[((code + i) << (9 - l)) + k] = (uint16_t)((l << 8) | h.vals[p + i]);
    code = (code + nb) << 1;
    p += nb;
  }
  t.maxcode[0] = t.maxcode[17] = -1;
}

bool info_consistent(const rpo_jpeg_info& f) {
  if (f.width < 1 || f.width > 65535 || f.height < 1 || f.height > 65535) return false;
  if (f.components == 1) { if (f.h_samp != 1 || f.v_samp != 1) return false; }
  else if (f.components == 3) {
    if (!((f.h_samp == 1 && f.v_samp == 1) || (f.h_samp == 2 && f.v_samp == 1) || (f.h_samp == 2 && f.v_samp == 2))) return false;
  } else return false;
  if (f.mcus_x != (f.width + 8 * f.h_samp - 1) / (8 * f.h_samp) || f.mcus_y != (f.height + 8 * f.v_samp - 1) / (8 * f.v_samp))
    return false;
  const int total = f.mcus_x * f.mcus_y;
  if (f.restart_interval < 0 || f.restart_interval > 65535) return false;
  if (f.units != (f.restart_interval ? (total + f.restart_interval - 1) / f.restart_interval : 1)) return false;
  if (f.table_bytes != (int64_t)sizeof(Tables) || f.coef_bytes != (int64_t)total * blocks_per_mcu(f) * 128) return false;
  if (f.scan_offset < 0 || f.scan_bytes < 0 || f.scan_bytes > 0x7fffffff) return false;
  return true;
}

constexpr int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

}  // namespace

extern "C" int rpo_jpeg_probe(const uint8_t* file, int64_t nbytes, rpo_jpeg_info* info) {
  if (!file || !info || nbytes <= 0) return RPO_E_BADARG;
  Parsed P;
  const int rc = parse_header(file, nbytes, P);
  *info = P.info;
  return rc;
}

extern "C" int rpo_jpeg_tables(const uint8_t* file, int64_t nbytes, void* blob, int64_t blob_bytes) {
  if (!file || !blob || nbytes <= 0) return RPO_E_BADARG;
  if (blob_bytes < (int64_t)sizeof(Tables)) return RPO_E_WORKSPACE;
  Parsed P;
  const int rc = parse_header(file, nbytes, P);
  if (rc) return rc;
  Tables* T = static_cast<Tables*>(blob);
  memset(T, 0, sizeof(Tables));
  for (int c = 0; c < P.info.components; ++c) {
    for (int k = 0; k < 64; ++k) T->quant[c][ZIGZAG_H[k]] = P.qtab[P.comp_q[c]][k];
    derive(P.huff[0][P.comp_dc[c]], T->dc[c]);
    derive(P.huff[1][P.comp_ac[c]], T->ac[c]);
  }
  return 0;
}

extern "C" size_t rpo_jpeg_workspace_bytes(rpo_jpeg_desc* descs, int n) {
  if (!descs || n <= 0 || n > 65535) return 0;
  int64_t units = 0;
  for (int i = 0; i < n; ++i) {
    if (!info_consistent(descs[i].info) || units + descs[i].info.units > 0x7fffffff) return 0;
    descs[i].unit_base = (int32_t)units;
    units += descs[i].info.units;
  }
  int64_t off = align_up(units * 4, 256);
  for (int i = 0; i < n; ++i) {
    descs[i].coef_offset = off;
    off += descs[i].info.coef_bytes;
  }
  return (size_t)off + 16;
}

extern "C" int rpo_jpeg_decode_batch(const uint8_t* files, int64_t files_bytes, const rpo_jpeg_desc* desc_host,
                                     const rpo_jpeg_desc* desc_dev, int n, uint8_t* out, int64_t out_bytes, void* workspace,
                                     size_t workspace_bytes, int32_t* status, void* stream) {
  if (!files || !desc_host || !desc_dev || !out || !workspace || !status || n <= 0 || files_bytes <= 0 || out_bytes <= 0)
    return RPO_E_BADARG;
  if (n > 65535) return RPO_E_SHAPE;
  if (reinterpret_cast<uintptr_t>(files) % 16 || reinterpret_cast<uintptr_t>(workspace) % 16) return RPO_E_ALIGN;
  int64_t units = 0, max_blocks = 1, max_pix = 1;
  for (int i = 0; i < n; ++i) {           // the descriptors are the only untrusted input of the launch: validate the host copy
    const rpo_jpeg_desc& d = desc_host[i];
    const rpo_jpeg_info& f = d.info;
    if (!info_consistent(f)) return RPO_E_SHAPE;
    if (d.file_offset < 0 || d.file_bytes <= 0 || d.file_offset + d.file_bytes > files_bytes ||
        f.scan_offset + f.scan_bytes > d.file_bytes)
      return RPO_E_SHAPE;
    if (d.table_offset < 0 || d.table_offset + f.table_bytes > files_bytes) return RPO_E_SHAPE;
    if (d.table_offset % 16) return RPO_E_ALIGN;
    if (d.out_offset < 0 || d.out_offset + (int64_t)f.width * f.height * 3 > out_bytes) return RPO_E_SHAPE;
    if ((int64_t)f.width * f.height > 0x7fffffff) return RPO_E_SHAPE;   // the colour kernel counts pixels in an int
    if (d.unit_base != units) return RPO_E_WORKSPACE;
    units += f.units;
    if (units > 0x7fffffff) return RPO_E_SHAPE;
    max_blocks = std::max<int64_t>(max_blocks, f.coef_bytes / 128);
    max_pix = std::max<int64_t>(max_pix, (int64_t)f.width * f.height);
  }
  int64_t off = align_up(units * 4, 256);
  for (int i = 0; i < n; ++i) {
    if (desc_host[i].coef_offset != off) return RPO_E_WORKSPACE;
    off += desc_host[i].info.coef_bytes;
  }
  if ((size_t)off + 16 > workspace_bytes) return RPO_E_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  hipLaunchKernelGGL(restart_scan_kernel, dim3(n), dim3(SCAN_THREADS), 0, s, files, desc_dev, reinterpret_cast<int32_t*>(ws),
                     status);
  const int lanes = (int)std::min<int64_t>(64, (units + 4095) / 4096);
  if (lanes == 1)
    hipLaunchKernelGGL(entropy_kernel<true>, dim3((unsigned)units), dim3(64), 0, s, files, files_bytes, desc_dev, n,
                       (int)units, lanes, ws, status);
  else
    hipLaunchKernelGGL(entropy_kernel<false>, dim3((unsigned)((units + lanes - 1) / lanes)), dim3(64), 0, s, files,
                       files_bytes, desc_dev, n, (int)units, lanes, ws, status);
  hipLaunchKernelGGL(idct_kernel, dim3((unsigned)std::min<int64_t>((max_blocks + 255) / 256, 64), n), dim3(256), 0, s, files,
                     desc_dev, ws);
  hipLaunchKernelGGL(colour_kernel, dim3((unsigned)std::min<int64_t>((max_pix + 255) / 256, 256), n), dim3(256), 0, s, desc_dev,
                     ws, out);
  return rpo_launch_status();
}

// ==== progressive (SOF2, Huffman) files ===============================================================================
// The same coefficient blocks, filled by several scans (ITU T.81 Annex G); IDCT and colour conversion are the kernels above.
// The arithmetic restated (G.1.2 / G.2; p1 = 1 << Al):
//   DC first        Huffman category s <= 11, pred += extend(bits(s)) modulo 2^32 per component (0 at a restart),
//                   coefficient 0 = low 16 bits of pred << Al
//   DC refinement   one raw bit per block: coefficient 0 |= p1
//   AC first        symbol (r, s): s != 0 -> skip r, coefficient k = extend(bits(s)) << Al; (15, 0) -> skip 16;
//                   (r < 15, 0) -> EOBRUN = (1 << r) + bits(r): this block's band ends here and EOBRUN - 1 further blocks are
//                   end-of-band; carried across blocks, 0 at a restart
//   AC refinement   symbol (r, 1) + sign bit: the new coefficient +-p1 lands on the (r + 1)-th still-zero coefficient; every
//                   nonzero coefficient passed on the way takes one correction bit, and a set bit whose p1 position is still
//                   clear moves it p1 away from zero; (15, 0) passes 16 zero coefficients; in end-of-band blocks the nonzero
//                   coefficients of [Ss, Se] still take their correction bits
// Interleaved DC scans walk the frame's MCUs; a scan of one component walks that component's own block grid in raster order
// (restart intervals count blocks there).  A UNIT is one restart interval of one scan; a scan's LEVEL is one more than the
// highest level among earlier scans sharing a component and a coefficient with it (<= 14 levels: one first scan and at
// most 13 refinements per coefficient).  The host walks all markers and the entropy-coded bytes between them
// (prog_parse: plain C++, never reads past nbytes), checks the scan script and writes the PLAN blob:
//   ProgHead (quantisation tables first, where idct_kernel expects Tables::quant) | ProgScan[nscans] | HuffTab[ntabs] as
//   derived at each SOS | int32 start[nunits]: file offset of the unit's first byte, -1 = its restart marker is missing
// prog_zero_kernel zeroes the coefficient blocks and the status words, prog_entropy_kernel runs once per level (kernel
// boundaries order the levels; one lane per unit, lanes of another level leave at once), then idct_kernel / colour_kernel.
// Bounds, as for the baseline kernel: block counts from the header; k strictly increases up to Se; EOBRUN <= 32767 and is
// consumed one block per iteration; every byte through Bits::byte_at inside [unit start, scan end); table indices masked.
namespace {

struct ProgHead {
  uint16_t quant[3][64];   // natural order; the same place as Tables::quant
  int32_t nscans, ntabs, nunits, blob_bytes;
};
struct ProgScan {
  int32_t unit0, nunits;   // this scan's units among the file's
  int32_t ri;              // restart interval in MCUs (interleaved) or blocks; 0 = none
  int32_t level;
  int32_t end;             // file offset behind the scan's entropy-coded bytes
  int16_t tab[4];          // HuffTab index: DC of comp[0..2], AC; -1 = not used
  uint8_t ncomp, comp[3];
  uint8_t ss, se, ah, al;
  int32_t pad[3];          // 48 bytes: the HuffTabs behind the scans stay 16-byte aligned
};
static_assert(sizeof(ProgHead) == 400 && sizeof(ProgScan) == 48 && offsetof(ProgHead, quant) == offsetof(Tables, quant),
              "plan layout");
constexpr int PROG_MAX_LEVELS = 14;

HD const ProgScan* prog_scans(const ProgHead* h) { return reinterpret_cast<const ProgScan*>(h + 1); }
HD const HuffTab* prog_tabs(const ProgHead* h) { return reinterpret_cast<const HuffTab*>(prog_scans(h) + h->nscans); }
HD const int32_t* prog_starts(const ProgHead* h) { return reinterpret_cast<const int32_t*>(prog_tabs(h) + h->ntabs); }
constexpr int64_t prog_blob_bytes(int64_t nscans, int64_t ntabs, int64_t nunits) {
  return ((int64_t)sizeof(ProgHead) + nscans * (int64_t)sizeof(ProgScan) + ntabs * (int64_t)sizeof(HuffTab) + nunits * 4 + 15) /
         16 * 16;
}

// blocks of component c across / down its own grid: ceil(ceil(W * h_c / h_max) / 8)
HD int comp_blocks_x(const rpo_jpeg_info& f, int c) {
  return ((c == 0 ? f.width : (f.width + f.h_samp - 1) / f.h_samp) + 7) >> 3;
}
HD int comp_blocks_y(const rpo_jpeg_info& f, int c) {
  return ((c == 0 ? f.height : (f.height + f.v_samp - 1) / f.v_samp) + 7) >> 3;
}
// block (bx, by) of component c in MCU order, as sample_at addresses it
HD int64_t block_index(const rpo_jpeg_info& f, int c, int bx, int by) {
  if (f.components == 1) return (int64_t)by * f.mcus_x + bx;
  const int hv = f.h_samp * f.v_samp;
  if (c == 0)
    return ((int64_t)(by / f.v_samp) * f.mcus_x + bx / f.h_samp) * (hv + 2) + (by % f.v_samp) * f.h_samp + bx % f.h_samp;
  return ((int64_t)by * f.mcus_x + bx) * (hv + 2) + hv + c - 1;
}

HD uint32_t take_bit(Bits& br) {
  br.refill();
  const uint32_t b = br.peek(1);
  br.skip(1);
  return b;
}

// a correction bit for an already nonzero coefficient
HD void refine_nonzero(Bits& br, i16a_t* p, int p1) {
  if (take_bit(br)) {
    const int v = *p;
    if ((v & p1) == 0) *p = (int16_t)(v >= 0 ? v + p1 : v - p1);
  }
}

struct ProgState {
  uint32_t pred[3];
  int eobrun;
};

// One block of one scan.  dc: the table of this block's component (DC first only); ac: the scan's AC table.
HD int prog_block(Bits& br, const ProgScan& sc, const HuffTab* dc, const HuffTab* ac, i16a_t* blk, ProgState& st, int ci) {
  const int al = sc.al & 15, p1 = 1 << al, ss = sc.ss & 63, se = sc.se & 63;
  if (se == 0) {
    if (sc.ah == 0) {                                                 // DC first
      br.refill();
      const int s = huff_symbol(br, dc);
      if (s < 0 || s > 11) return RPO_JPEG_BAD_CODE;
      if (s) {
        const uint32_t diff = (uint32_t)extend(br.peek(s), s);
        br.skip(s);
        if (ci == 0) st.pred[0] += diff; else if (ci == 1) st.pred[1] += diff; else st.pred[2] += diff;
      }
      blk[0] = (int16_t)(uint16_t)((ci == 0 ? st.pred[0] : ci == 1 ? st.pred[1] : st.pred[2]) << al);
    } else {                                                          // DC refinement
      if (take_bit(br)) blk[0] = (int16_t)(blk[0] | p1);
    }
  } else if (sc.ah == 0) {                                            // AC first
    if (st.eobrun > 0) {
      --st.eobrun;
      return RPO_JPEG_OK;
    }
    for (int k = ss; k <= se;) {                                      // k grows by >= 1 per iteration
      br.refill();
      const int rs = huff_symbol(br, ac);
      if (rs < 0) return RPO_JPEG_BAD_CODE;
      const int r = rs >> 4, s = rs & 15;
      if (s) {
        k += r;
        if (k > se) return RPO_JPEG_BAD_INDEX;
        blk[zigzag(k)] = (int16_t)(uint16_t)((uint32_t)extend(br.peek(s), s) << al);
        br.skip(s);
        ++k;
      } else if (r == 15) {
        k += 16;
      } else {
        st.eobrun = 1 << r;
        if (r) {
          st.eobrun += (int)br.peek(r);
          br.skip(r);
        }
        --st.eobrun;                                                  // this block is the first of the run
        break;
      }
    }
  } else {                                                            // AC refinement
    int k = ss;
    if (st.eobrun == 0) {
      for (; k <= se; ++k) {                                          // k grows by >= 1 per iteration
        br.refill();
        const int rs = huff_symbol(br, ac);
        if (rs < 0) return RPO_JPEG_BAD_CODE;
        int r = rs >> 4;
        const int s = rs & 15;
        int val = 0;
        if (s) {
          if (s != 1) return RPO_JPEG_BAD_CODE;
          val = br.peek(1) ? p1 : -p1;
          br.skip(1);
        } else if (r != 15) {
          st.eobrun = 1 << r;
          if (r) {
            st.eobrun += (int)br.peek(r);
            br.skip(r);
          }
          break;                                                      // the rest of this block is end-of-band, below
        }
        for (; k <= se; ++k) {                                        // pass r zero coefficients, stop on the next one
          i16a_t* p = blk + zigzag(k);
          if (*p != 0) refine_nonzero(br, p, p1);
          else if (--r < 0) break;
        }
        if (s) {
          if (k > se) return RPO_JPEG_BAD_INDEX;
          blk[zigzag(k)] = (int16_t)val;
        }
      }
    }
    if (st.eobrun > 0) {
      for (; k <= se; ++k) {
        i16a_t* p = blk + zigzag(k);
        if (*p != 0) refine_nonzero(br, p, p1);
      }
      --st.eobrun;
    }
  }
  return br.overrun() ? RPO_JPEG_TRUNCATED : RPO_JPEG_OK;
}

// Unit `unit` of scan sc of image d, starting at file offset `start` (< 0: its restart marker was not found).  tab[0..2]: DC
// tables of the scan's components, tab[3]: its AC table.  Returns the RPO_JPEG_* status; what follows an error stays as it was.
HD int prog_decode_unit(const uint8_t* files, int64_t files_bytes, const rpo_jpeg_desc& d, const ProgScan& sc,
                        const HuffTab* const* tab, int16_t* coef, int unit, int start) {
  const rpo_jpeg_info& f = d.info;
  if (start < 0) return RPO_JPEG_NO_RESTART;
  const int nsc = min((int)sc.ncomp, f.components);
  const bool interleaved = nsc > 1;
  const int c0 = min((int)sc.comp[0], f.components - 1);
  const int bw = comp_blocks_x(f, c0);
  const int total = interleaved ? f.mcus_x * f.mcus_y : bw * comp_blocks_y(f, c0);
  const int ri = sc.ri > 0 ? sc.ri : total;
  const int64_t first = (int64_t)unit * ri;
  if (unit < 0 || first >= total) return RPO_JPEG_OK;
  const int count = (int)min((int64_t)ri, total - first);
  const int64_t end = d.file_offset + min(max((int64_t)sc.end, (int64_t)0), d.file_bytes);
  Bits br;
  br.init(files, min(d.file_offset + start, end), end, files_bytes);
  ProgState st = {{0, 0, 0}, 0};
  for (int m = (int)first; m < (int)first + count; ++m) {
    // an interleaved MCU holds h x v blocks of each of the scan's components; a scan of one component walks single blocks
    // of its own grid.  ONE call site of prog_block, so that its four decoders are in the kernel once.
    const int mx = interleaved ? m % f.mcus_x : m % bw, my = interleaved ? m / f.mcus_x : m / bw;
    for (int i = 0; i < nsc; ++i) {
      const int c = min((int)(i == 0 ? sc.comp[0] : i == 1 ? sc.comp[1] : sc.comp[2]), f.components - 1);
      const int h = interleaved && c == 0 ? f.h_samp : 1, v = interleaved && c == 0 ? f.v_samp : 1;
      const HuffTab* dc = i == 0 ? tab[0] : i == 1 ? tab[1] : tab[2];
      for (int j = 0; j < h * v; ++j) {
        i16a_t* blk = coef + block_index(f, c, mx * h + j % h, my * v + j / h) * 64;
        const int err = prog_block(br, sc, dc, tab[3], blk, st, i);
        if (err) return err;
      }
    }
  }
  return RPO_JPEG_OK;
}

// the scan that holds unit `unit` of the file: last scan with unit0 <= unit
HD int prog_scan_of(const ProgHead* h, int unit) {
  const ProgScan* sc = prog_scans(h);
  int lo = 0, hi = h->nscans - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (sc[mid].unit0 <= unit) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void prog_zero_kernel(char* ws, int64_t nwords16, int32_t* status, int n) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) status[t] = RPO_JPEG_OK;
  int4a_t* p = reinterpret_cast<int4a_t*>(ws);
  for (int64_t i = t; i < nwords16; i += (int64_t)gridDim.x * blockDim.x) p[i] = int4{0, 0, 0, 0};
}

// The units of dependency level `level`: the lane layout of entropy_kernel over ALL units of the batch; a unit of another
// level returns at once.  ONE_PER_BLOCK: one unit per wave, the scan's (at most four) Huffman tables copied to LDS.
template <bool ONE_PER_BLOCK>
__global__ __launch_bounds__(64) void prog_entropy_kernel(const uint8_t* __restrict__ files, int64_t files_bytes,
                                                          const rpo_jpeg_desc* __restrict__ desc, int n, int total_units,
                                                          int lanes, int level, char* ws, int32_t* status) {
  __shared__ int4 lds_tab[ONE_PER_BLOCK ? 4 * sizeof(HuffTab) / 16 : 1];
  if (!ONE_PER_BLOCK && (int)threadIdx.x >= lanes) return;
  const int u = ONE_PER_BLOCK ? (int)blockIdx.x : blockIdx.x * lanes + threadIdx.x;
  if (u >= total_units) return;                            // block-uniform when ONE_PER_BLOCK, as everything up to the copy
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (desc[mid].unit_base <= u) lo = mid; else hi = mid - 1;
  }
  const rpo_jpeg_desc d = desc[lo];
  const int unit = u - d.unit_base;
  if (unit >= d.info.units) return;
  const ProgHead* head = reinterpret_cast<const ProgHead*>(files + d.table_offset);
  if (head->nunits != d.info.units || head->blob_bytes != d.info.table_bytes || head->nscans < 1 || head->ntabs < 0 ||
      prog_blob_bytes(head->nscans, head->ntabs, head->nunits) != d.info.table_bytes) {
    if (threadIdx.x == 0 || !ONE_PER_BLOCK) atomicMax(status + lo, RPO_JPEG_BAD_CODE);   // not this file's plan
    return;
  }
  const ProgScan sc = prog_scans(head)[prog_scan_of(head, unit)];
  if (sc.level != level) return;
  const HuffTab* tab[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int t = sc.tab[i];
    tab[i] = prog_tabs(head) + (t >= 0 && t < head->ntabs ? t : 0);
  }
  if (ONE_PER_BLOCK) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (sc.tab[i] < 0) continue;
      const int4* src = reinterpret_cast<const int4*>(tab[i]);
      int4* dst = lds_tab + i * (int)(sizeof(HuffTab) / 16);
      for (int k = threadIdx.x; k < (int)(sizeof(HuffTab) / 16); k += 64) dst[k] = src[k];
      tab[i] = reinterpret_cast<const HuffTab*>(dst);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
  }
  const int err = prog_decode_unit(files, files_bytes, d, sc, tab, reinterpret_cast<int16_t*>(ws + d.coef_offset),
                                   unit - sc.unit0, prog_starts(head)[unit]);
  if (err) atomicMax(status + lo, err);
}

// ---- host: the marker walk of a progressive file ------------------------------------------------------------------
struct ProgPlan {
  Parsed P;                        // info, quantisation tables, the Huffman tables as last defined
  int comp_q[3];
  std::vector<ProgScan> scans;
  std::vector<HuffTab> tabs;
  std::vector<int32_t> starts;
  int levels;
};

int prog_parse(const uint8_t* p, int64_t n, ProgPlan& G) {
  Parsed& P = G.P;
  memset(&P, 0, sizeof(P));
  G.scans.clear(); G.tabs.clear(); G.starts.clear(); G.levels = 0;
  if (n < 4 || p[0] != 0xFF || p[1] != 0xD8) return RPO_E_JPEG_CORRUPT;
  if (n > 0x7fffffff) return RPO_E_SHAPE;                  // unit starts are int32 file offsets
  int64_t pos = 2;
  bool have_frame = false, jfif = false;
  int adobe = -1, nc = 0, ri = 0;
  uint8_t cid[4] = {0}, ch[4] = {0}, cv[4] = {0}, cq[4] = {0};
  int8_t al[3][64], lvl[3][64];                            // per (component, coefficient): Al reached, level of its last scan
  memset(al, -1, sizeof(al)); memset(lvl, -1, sizeof(lvl));
  int tabidx[2][4];                                        // the derived copy of the CURRENT definition of (class, id), or -1
  memset(tabidx, -1, sizeof(tabidx));
  rpo_jpeg_info& f = P.info;
  for (;;) {
    if (pos + 2 > n) {                                     // the file ends without EOI: the scans so far are the script
      if (G.scans.empty()) return RPO_E_JPEG_CORRUPT;
      break;
    }
    if (p[pos] != 0xFF) return RPO_E_JPEG_CORRUPT;
    const int m = p[pos + 1];
    pos += 2;
    if (m == 0xFF) { pos -= 1; continue; }
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
    if (m == 0xD9) {
      if (G.scans.empty()) return RPO_E_JPEG_CORRUPT;
      break;
    }
    if (m == 0xD8) return RPO_E_JPEG_CORRUPT;
    if (pos + 2 > n) return RPO_E_JPEG_CORRUPT;
    const int L = (p[pos] << 8) | p[pos + 1];
    if (L < 2 || pos + L > n) return RPO_E_JPEG_CORRUPT;
    const uint8_t* seg = p + pos + 2;
    const int sl = L - 2;
    pos += L;
    if (m == 0xC0 || m == 0xC1) return RPO_E_JPEG_SEQUENTIAL;
    if (m >= 0xC9 && m <= 0xCF) return RPO_E_JPEG_ARITHMETIC;   // SOF9..15 and DAC
    if (m == 0xC3 || m == 0xC5 || m == 0xC6 || m == 0xC7) return RPO_E_JPEG_LOSSLESS;
    if (m == 0xC2) {
      if (have_frame || sl < 6) return RPO_E_JPEG_CORRUPT;
      if (seg[0] != 8) return RPO_E_JPEG_PRECISION;
      f.height = (seg[1] << 8) | seg[2];
      f.width = (seg[3] << 8) | seg[4];
      nc = seg[5];
      if (sl != 6 + 3 * nc || f.height == 0 || f.width == 0) return RPO_E_JPEG_CORRUPT;
      if (nc != 1 && nc != 3) return RPO_E_JPEG_COMPONENTS;
      for (int i = 0; i < nc; ++i) {
        cid[i] = seg[6 + 3 * i]; ch[i] = seg[7 + 3 * i] >> 4; cv[i] = seg[7 + 3 * i] & 15; cq[i] = seg[8 + 3 * i];
        if (cq[i] > 3 || ch[i] == 0 || cv[i] == 0) return RPO_E_JPEG_CORRUPT;
      }
      f.components = nc;
      have_frame = true;
    } else if (m == 0xDB) {
      if (!G.scans.empty()) return RPO_E_JPEG_SCRIPT;      // the IDCT has one table per component
      const int rc = parse_dqt(seg, sl, P);
      if (rc) return rc;
    } else if (m == 0xC4) {
      for (int q = 0; q + 17 <= sl;) {                     // the ids this segment redefines (parse_dht validates it)
        int cnt = 0;
        for (int i = 1; i <= 16; ++i) cnt += seg[q + i];
        if ((seg[q] >> 4) <= 1 && (seg[q] & 15) <= 3) tabidx[seg[q] >> 4][seg[q] & 15] = -1;
        q += 17 + cnt;
      }
      const int rc = parse_dht(seg, sl, P);
      if (rc) return rc;
    } else if (m == 0xDD) {
      if (sl != 2) return RPO_E_JPEG_CORRUPT;
      ri = (seg[0] << 8) | seg[1];
    } else if (m == 0xE0) {
      if (sl >= 5 && memcmp(seg, "JFIF\0", 5) == 0) jfif = true;
    } else if (m == 0xEE) {
      if (sl >= 12 && memcmp(seg, "Adobe", 5) == 0) adobe = seg[11];
    } else if (m == 0xDA) {
      if (!have_frame) return RPO_E_JPEG_CORRUPT;
      const int ns = sl > 0 ? seg[0] : 0;
      if (ns < 1 || ns > 4 || sl != 4 + 2 * ns) return RPO_E_JPEG_CORRUPT;
      if (G.scans.empty()) {                               // the frame's colour and sampling rules, as parse_header's
        f.h_samp = f.v_samp = 1;
        if (nc == 3) {
          const bool rgb_ids = cid[0] == 'R' && cid[1] == 'G' && cid[2] == 'B';
          if (!jfif && (adobe == 0 || (adobe < 0 && rgb_ids))) return RPO_E_JPEG_RGB;
          if (ch[1] != 1 || cv[1] != 1 || ch[2] != 1 || cv[2] != 1) return RPO_E_JPEG_SAMPLING;
          if (!((ch[0] == 1 && cv[0] == 1) || (ch[0] == 2 && cv[0] == 1) || (ch[0] == 2 && cv[0] == 2)))
            return RPO_E_JPEG_SAMPLING;
          f.h_samp = ch[0];
          f.v_samp = cv[0];
        }
        for (int i = 0; i < nc; ++i) {
          if (!P.qset[cq[i]]) return RPO_E_JPEG_CORRUPT;
          G.comp_q[i] = cq[i];
        }
        f.mcus_x = (f.width + 8 * f.h_samp - 1) / (8 * f.h_samp);
        f.mcus_y = (f.height + 8 * f.v_samp - 1) / (8 * f.v_samp);
        f.scan_offset = pos;
        f.scan_bytes = n - pos;
        f.coef_bytes = (int64_t)f.mcus_x * f.mcus_y * blocks_per_mcu(f) * 128;
      }
      ProgScan sc;
      memset(&sc, 0, sizeof(sc));
      sc.tab[0] = sc.tab[1] = sc.tab[2] = sc.tab[3] = -1;
      sc.ncomp = (uint8_t)ns;
      sc.ss = seg[1 + 2 * ns]; sc.se = seg[2 + 2 * ns]; sc.ah = seg[3 + 2 * ns] >> 4; sc.al = seg[3 + 2 * ns] & 15;
      if (ns > nc) return RPO_E_JPEG_SCRIPT;
      int td[3] = {0, 0, 0}, ta[3] = {0, 0, 0}, prev = -1;
      for (int i = 0; i < ns; ++i) {                       // the scan's components: the frame's, in the frame's order
        int c = -1;
        for (int j = 0; j < nc; ++j)
          if (seg[1 + 2 * i] == cid[j]) { c = j; break; }
        if (c < 0 || c <= prev) return RPO_E_JPEG_CORRUPT;
        prev = c;
        sc.comp[i] = (uint8_t)c;
        td[i] = seg[2 + 2 * i] >> 4; ta[i] = seg[2 + 2 * i] & 15;
        if (td[i] > 3 || ta[i] > 3) return RPO_E_JPEG_CORRUPT;
      }
      // ---- the script rules
      const bool dc_scan = sc.ss == 0;
      if (sc.ah > 13 || sc.al > 13 || sc.se > 63 || sc.ss > sc.se) return RPO_E_JPEG_SCRIPT;
      if (dc_scan ? sc.se != 0 : ns != 1) return RPO_E_JPEG_SCRIPT;
      int level = 0;
      for (int i = 0; i < ns; ++i) {
        const int c = sc.comp[i];
        if (!dc_scan && al[c][0] < 0) return RPO_E_JPEG_SCRIPT;              // AC before the component's DC first scan
        for (int k = sc.ss; k <= sc.se; ++k) {
          if (al[c][k] < 0 ? sc.ah != 0 : (sc.ah != al[c][k] || sc.al != sc.ah - 1)) return RPO_E_JPEG_SCRIPT;
          al[c][k] = (int8_t)sc.al;
          level = std::max(level, lvl[c][k] + 1);
        }
      }
      if (level >= PROG_MAX_LEVELS) return RPO_E_JPEG_SCRIPT;                // cannot happen: Al falls by one per level
      for (int i = 0; i < ns; ++i)
        for (int k = sc.ss; k <= sc.se; ++k) lvl[sc.comp[i]][k] = (int8_t)level;
      sc.level = level;
      G.levels = std::max(G.levels, level + 1);
      // ---- the tables this scan reads, as defined now
      for (int i = 0; i < ns; ++i) {
        const int tc = dc_scan ? 0 : 1, th = dc_scan ? td[i] : ta[i];
        if (dc_scan && sc.ah != 0) break;                                    // DC refinement: raw bits only
        if (!P.huff[tc][th].set) return RPO_E_JPEG_CORRUPT;
        if (tabidx[tc][th] < 0) {
          if (G.tabs.size() >= 32767) return RPO_E_JPEG_SCRIPT;
          G.tabs.emplace_back();
          derive(P.huff[tc][th], G.tabs.back());
          tabidx[tc][th] = (int)G.tabs.size() - 1;
        }
        sc.tab[dc_scan ? i : 3] = (int16_t)tabidx[tc][th];
      }
      // ---- its units
      const int c0 = sc.comp[0];
      const int64_t total = ns > 1 ? (int64_t)f.mcus_x * f.mcus_y : (int64_t)comp_blocks_x(f, c0) * comp_blocks_y(f, c0);
      sc.ri = ri;
      const int64_t units = ri ? (total + ri - 1) / ri : 1;
      if ((int64_t)G.starts.size() + units > 0x7fffffff / 8) return RPO_E_SHAPE;
      sc.unit0 = (int32_t)G.starts.size();
      sc.nunits = (int32_t)units;
      G.starts.resize(G.starts.size() + (size_t)units, -1);
      int32_t* st = G.starts.data() + sc.unit0;
      st[0] = (int32_t)pos;
      int64_t ord = 0;
      while (pos < n) {                                    // to the marker that ends the scan, or the end of the file
        if (p[pos] != 0xFF) { ++pos; continue; }
        if (pos + 1 >= n) { pos = n; break; }
        const int b = p[pos + 1];
        if (b == 0) { pos += 2; continue; }                // a stuffed FF
        if (b == 0xFF) { ++pos; continue; }                // fill byte
        if (b >= 0xD0 && b <= 0xD7) {
          if (++ord < units) st[ord] = (int32_t)(pos + 2);
          pos += 2;
          continue;
        }
        break;
      }
      // the decoder stops at the first FF that is no stuffed FF: fill bytes in front of the marker included
      sc.end = (int32_t)pos;
      G.scans.push_back(sc);
    }
    // every other segment (APPn, COM, DNL, ...) is skipped
  }
  for (int c = 0; c < nc; ++c)
    for (int k = 0; k < 64; ++k)
      if (al[c][k] != 0) return RPO_E_JPEG_SCRIPT;         // incomplete: libjpeg would smooth the blocks
  f.restart_interval = 0;                                  // per scan here
  f.units = (int32_t)G.starts.size();
  f.reserved = G.levels;
  f.table_bytes = prog_blob_bytes((int64_t)G.scans.size(), (int64_t)G.tabs.size(), (int64_t)G.starts.size());
  return 0;
}

bool prog_info_consistent(const rpo_jpeg_info& f) {
  rpo_jpeg_info g = f;                                     // the geometry rules are the baseline's
  g.restart_interval = 0; g.units = 1; g.table_bytes = sizeof(Tables);
  if (!info_consistent(g)) return false;
  if (f.units < 1 || f.reserved < 1 || f.reserved > PROG_MAX_LEVELS) return false;
  if (f.table_bytes < prog_blob_bytes(1, 0, 1) || f.table_bytes % 16 || f.table_bytes > 0x7fffffff) return false;
  return true;
}

}  // namespace

extern "C" int rpo_jpeg_prog_probe(const uint8_t* file, int64_t nbytes, rpo_jpeg_info* info) {
  if (!file || !info || nbytes <= 0) return RPO_E_BADARG;
  ProgPlan G;
  const int rc = prog_parse(file, nbytes, G);
  *info = G.P.info;
  return rc;
}

extern "C" int rpo_jpeg_prog_plan(const uint8_t* file, int64_t nbytes, void* blob, int64_t blob_bytes) {
  if (!file || !blob || nbytes <= 0) return RPO_E_BADARG;
  ProgPlan G;
  const int rc = prog_parse(file, nbytes, G);
  if (rc) return rc;
  if (blob_bytes < G.P.info.table_bytes) return RPO_E_WORKSPACE;
  memset(blob, 0, (size_t)G.P.info.table_bytes);
  ProgHead* H = static_cast<ProgHead*>(blob);
  for (int c = 0; c < G.P.info.components; ++c)
    for (int k = 0; k < 64; ++k) H->quant[c][ZIGZAG_H[k]] = G.P.qtab[G.comp_q[c]][k];
  H->nscans = (int32_t)G.scans.size();
  H->ntabs = (int32_t)G.tabs.size();
  H->nunits = (int32_t)G.starts.size();
  H->blob_bytes = (int32_t)G.P.info.table_bytes;
  char* q = reinterpret_cast<char*>(H + 1);
  memcpy(q, G.scans.data(), G.scans.size() * sizeof(ProgScan));
  q += G.scans.size() * sizeof(ProgScan);
  if (!G.tabs.empty()) memcpy(q, G.tabs.data(), G.tabs.size() * sizeof(HuffTab));
  q += G.tabs.size() * sizeof(HuffTab);
  memcpy(q, G.starts.data(), G.starts.size() * 4);
  return 0;
}

extern "C" size_t rpo_jpeg_prog_workspace_bytes(rpo_jpeg_desc* descs, int n) {
  if (!descs || n <= 0 || n > 65535) return 0;
  int64_t units = 0, off = 0;
  for (int i = 0; i < n; ++i) {
    if (!prog_info_consistent(descs[i].info) || units + descs[i].info.units > 0x7fffffff) return 0;
    descs[i].unit_base = (int32_t)units;
    units += descs[i].info.units;
    descs[i].coef_offset = off;
    off += descs[i].info.coef_bytes;
  }
  return (size_t)off + 16;
}

extern "C" int rpo_jpeg_prog_decode_batch(const uint8_t* files, int64_t files_bytes, const rpo_jpeg_desc* desc_host,
                                          const rpo_jpeg_desc* desc_dev, int n, uint8_t* out, int64_t out_bytes,
                                          void* workspace, size_t workspace_bytes, int32_t* status, void* stream) {
  if (!files || !desc_host || !desc_dev || !out || !workspace || !status || n <= 0 || files_bytes <= 0 || out_bytes <= 0)
    return RPO_E_BADARG;
  if (n > 65535) return RPO_E_SHAPE;
  if (reinterpret_cast<uintptr_t>(files) % 16 || reinterpret_cast<uintptr_t>(workspace) % 16) return RPO_E_ALIGN;
  int64_t units = 0, max_blocks = 1, max_pix = 1, off = 0;
  int levels = 1;
  for (int i = 0; i < n; ++i) {           // as in rpo_jpeg_decode_batch: the host copy of every descriptor is validated
    const rpo_jpeg_desc& d = desc_host[i];
    const rpo_jpeg_info& f = d.info;
    if (!prog_info_consistent(f)) return RPO_E_SHAPE;
    if (d.file_offset < 0 || d.file_bytes <= 0 || d.file_bytes > 0x7fffffff || d.file_offset + d.file_bytes > files_bytes ||
        f.scan_offset + f.scan_bytes > d.file_bytes)
      return RPO_E_SHAPE;
    if (d.table_offset < 0 || d.table_offset + f.table_bytes > files_bytes) return RPO_E_SHAPE;
    if (d.table_offset % 16) return RPO_E_ALIGN;
    if (d.out_offset < 0 || d.out_offset + (int64_t)f.width * f.height * 3 > out_bytes) return RPO_E_SHAPE;
    if ((int64_t)f.width * f.height > 0x7fffffff) return RPO_E_SHAPE;
    if (d.unit_base != units || d.coef_offset != off) return RPO_E_WORKSPACE;
    units += f.units;
    off += f.coef_bytes;
    if (units > 0x7fffffff) return RPO_E_SHAPE;
    levels = std::max(levels, (int)f.reserved);
    max_blocks = std::max<int64_t>(max_blocks, f.coef_bytes / 128);
    max_pix = std::max<int64_t>(max_pix, (int64_t)f.width * f.height);
  }
  if ((size_t)off + 16 > workspace_bytes) return RPO_E_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  const int64_t words = off / 16;                           // coef_bytes is a multiple of 128
  const int64_t zthreads = std::max<int64_t>(words, n);
  hipLaunchKernelGGL(prog_zero_kernel, dim3((unsigned)std::min<int64_t>((zthreads + 255) / 256, 65536)), dim3(256), 0, s, ws,
                     words, status, n);
  const int lanes = (int)std::min<int64_t>(64, (units + 4095) / 4096);
  for (int level = 0; level < levels; ++level) {
    if (lanes == 1)
      hipLaunchKernelGGL(prog_entropy_kernel<true>, dim3((unsigned)units), dim3(64), 0, s, files, files_bytes, desc_dev, n,
                         (int)units, lanes, level, ws, status);
    else
      hipLaunchKernelGGL(prog_entropy_kernel<false>, dim3((unsigned)((units + lanes - 1) / lanes)), dim3(64), 0, s, files,
                         files_bytes, desc_dev, n, (int)units, lanes, level, ws, status);
  }
  hipLaunchKernelGGL(idct_kernel, dim3((unsigned)std::min<int64_t>((max_blocks + 255) / 256, 64), n), dim3(256), 0, s, files,
                     desc_dev, ws);
  hipLaunchKernelGGL(colour_kernel, dim3((unsigned)std::min<int64_t>((max_pix + 255) / 256, 256), n), dim3(256), 0, s, desc_dev,
                     ws, out);
  return rpo_launch_status();
}
