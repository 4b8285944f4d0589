// The JPEG decoder's own code on the CPU: rpo_amd/csrc/jpeg.hip is included as it stands and its __host__ __device__
// functions -- parse_header / rpo_jpeg_tables, the restart offsets as restart_scan_kernel derives them, decode_unit per
// unit, idct_block per block, pixel_rgb per pixel -- run here in plain C++.  Nothing calls the HIP runtime, so the program
// needs no GPU and can be built with the host sanitizers (tests/test_jpeg_streams_host.py builds it without them).
//
//   jpeg_host_decode IN OUT
// IN : int32 n, then per file int64 nbytes + the bytes.
// OUT: per file int32 x 12 = probe code, device status, width, height, components, h_samp, v_samp, restart interval,
//      units, scan_offset, mcus_x, mcus_y, then (probe code 0 only) height * width * 3 bytes of RGB.
// Each file is decoded from a heap buffer of exactly nbytes (16-byte aligned, as the device's file buffer is) and the
// coefficient workspace is exactly coef_bytes, so an address sanitizer sees every byte read or written outside them.
// build: hipcc -x hip --cuda-host-only -O1 -std=c++17 tests/host/jpeg_host_decode.cpp -o jpeg_host_decode
#include "../../rpo_amd/csrc/jpeg.hip"

#include <stdio.h>
#include <stdlib.h>

#include <vector>

namespace {

// what the four kernels do for ONE descriptor; returns the status word
int decode_file(const uint8_t* file, int64_t nbytes, const rpo_jpeg_info& f, const Tables* tab, uint8_t* rgb) {
  rpo_jpeg_desc d;
  memset(&d, 0, sizeof(d));
  d.info = f;
  d.file_bytes = nbytes;
  // restart_scan_kernel
  std::vector<int32_t> rst((size_t)f.units);
  for (int u = 0; u < f.units; ++u) rst[u] = u == 0 ? 0 : -1;
  if (f.units > 1) {
    const uint8_t* p = file + f.scan_offset;
    int ord = 0;
    for (int64_t i = 0; i < f.scan_bytes - 1; ++i)
      if (rst_at(p, i)) {
        if (ord + 1 < f.units) rst[ord + 1] = (int32_t)(i + 2);
        ++ord;
      }
  }
  // entropy_kernel
  int16_t* coef = static_cast<int16_t*>(aligned_alloc(16, (size_t)f.coef_bytes));
  if (!coef) return -1;
  int status = RPO_JPEG_OK;
  for (int u = 0; u < f.units; ++u) status = std::max(status, decode_unit(file, nbytes, d, tab, coef, u, rst[u]));
  // idct_kernel
  const int bpm = blocks_per_mcu(f), luma = bpm == 1 ? 1 : bpm - 2;
  const int nblk = f.mcus_x * f.mcus_y * bpm;
  for (int i = 0; i < nblk; ++i) {
    const int j = i % bpm;
    idct_block(coef + (int64_t)i * 64, tab->quant[j < luma ? 0 : j - luma + 1]);
  }
  // colour_kernel
  const int W = f.width;
  const int64_t npix = (int64_t)W * f.height;
  for (int64_t i = 0; i < npix; ++i) pixel_rgb(reinterpret_cast<const uint8_t*>(coef), f, (int)(i % W), (int)(i / W), rgb + i * 3);
  free(coef);
  return status;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int32_t n = 0;
  if (fread(&n, 4, 1, in) != 1) return 2;
  for (int k = 0; k < n; ++k) {
    int64_t nbytes = 0;
    if (fread(&nbytes, 8, 1, in) != 1 || nbytes <= 0) return 2;
    uint8_t* file = static_cast<uint8_t*>(malloc((size_t)nbytes));
    if (!file || fread(file, 1, (size_t)nbytes, in) != (size_t)nbytes) return 2;
    rpo_jpeg_info f;
    int32_t rec[12] = {rpo_jpeg_probe(file, nbytes, &f), -1, f.width, f.height, f.components, f.h_samp, f.v_samp,
                       f.restart_interval, f.units, (int32_t)f.scan_offset, f.mcus_x, f.mcus_y};
    std::vector<uint8_t> rgb;
    if (rec[0] == 0) {
      Tables* tab = static_cast<Tables*>(aligned_alloc(16, sizeof(Tables)));
      if (!tab || rpo_jpeg_tables(file, nbytes, tab, sizeof(Tables)) != 0 || !info_consistent(f)) return 3;
      rgb.resize((size_t)f.width * f.height * 3);
      rec[1] = decode_file(file, nbytes, f, tab, rgb.data());
      free(tab);
    }
    fwrite(rec, 4, 12, out);
    if (!rgb.empty()) fwrite(rgb.data(), 1, rgb.size(), out);
    free(file);
  }
  fclose(in);
  if (fclose(out) != 0) return 2;
  printf("decoded %d files\n", n);
  return 0;
}
