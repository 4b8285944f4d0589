// The progressive JPEG decoder's own code on the CPU: rpo_amd/csrc/jpeg.hip is included as it stands and rpo_jpeg_prog_probe,
// rpo_jpeg_prog_plan, prog_decode_unit for every unit in level order, idct_block per block and pixel_rgb per pixel run here
// in plain C++.  Nothing calls the HIP runtime, so the program needs no GPU and can be built with the host sanitizers.
// A file the progressive probe answers with RPO_E_JPEG_SEQUENTIAL is decoded through the baseline functions instead, as
// tests/host/jpeg_host_decode.cpp does, so a progressive file and its baseline twin can be compared inside one program.
//
//   jpeg_prog_host_decode IN OUT [probe]
// IN : int32 n, then per file int64 nbytes + the bytes.
// OUT: per file int32 x 12 = progressive probe code, device status, width, height, components, h_samp, v_samp, levels,
//      units, scan_offset, table_bytes, baseline probe code (only after RPO_E_JPEG_SEQUENTIAL, else 1), then -- if one of the
//      two probes accepted the file and `probe` was not given -- height * width * 3 bytes of RGB.
// Each file is probed and decoded from a heap buffer of exactly nbytes, the plan blob is exactly table_bytes and the
// coefficient workspace exactly coef_bytes, so an address sanitizer sees every byte read or written outside them.
// build: hipcc -x hip --offload-arch=gfx950 -O1 -std=c++17 tests/host/jpeg_prog_host_decode.cpp -o jpeg_prog_host_decode
#include "../../rpo_amd/csrc/jpeg.hip"

#include <stdio.h>
#include <stdlib.h>

#include <vector>

namespace {

void pixels(int16_t* coef, const rpo_jpeg_info& f, const uint16_t (*quant)[64], uint8_t* rgb) {
  const int bpm = blocks_per_mcu(f), luma = bpm == 1 ? 1 : bpm - 2;
  const int nblk = f.mcus_x * f.mcus_y * bpm;
  for (int i = 0; i < nblk; ++i) {                                    // idct_kernel
    const int j = i % bpm;
    idct_block(coef + (int64_t)i * 64, quant[j < luma ? 0 : j - luma + 1]);
  }
  const int W = f.width;                                              // colour_kernel
  const int64_t npix = (int64_t)W * f.height;
  for (int64_t i = 0; i < npix; ++i) pixel_rgb(reinterpret_cast<const uint8_t*>(coef), f, (int)(i % W), (int)(i / W), rgb + i * 3);
}

// what rpo_jpeg_prog_decode_batch's kernels do for ONE descriptor; returns the status word
int decode_progressive(const uint8_t* file, int64_t nbytes, const rpo_jpeg_info& f, const ProgHead* head, uint8_t* rgb) {
  rpo_jpeg_desc d;
  memset(&d, 0, sizeof(d));
  d.info = f;
  d.file_bytes = nbytes;
  int16_t* coef = static_cast<int16_t*>(aligned_alloc(16, (size_t)f.coef_bytes));
  if (!coef) return -1;
  memset(coef, 0, (size_t)f.coef_bytes);                              // prog_zero_kernel
  int status = RPO_JPEG_OK;
  if (head->nunits != f.units || head->blob_bytes != f.table_bytes) return -2;
  for (int level = 0; level < f.reserved; ++level)                    // prog_entropy_kernel, one launch per level
    for (int unit = 0; unit < f.units; ++unit) {
      const ProgScan sc = prog_scans(head)[prog_scan_of(head, unit)];
      if (sc.level != level) continue;
      const HuffTab* tab[4];
      for (int i = 0; i < 4; ++i) tab[i] = prog_tabs(head) + (sc.tab[i] >= 0 && sc.tab[i] < head->ntabs ? sc.tab[i] : 0);
      status = std::max(status, prog_decode_unit(file, nbytes, d, sc, tab, coef, unit - sc.unit0, prog_starts(head)[unit]));
    }
  pixels(coef, f, head->quant, rgb);
  free(coef);
  return status;
}

int decode_baseline(const uint8_t* file, int64_t nbytes, const rpo_jpeg_info& f, const Tables* tab, uint8_t* rgb) {
  rpo_jpeg_desc d;
  memset(&d, 0, sizeof(d));
  d.info = f;
  d.file_bytes = nbytes;
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
  int16_t* coef = static_cast<int16_t*>(aligned_alloc(16, (size_t)f.coef_bytes));
  if (!coef) return -1;
  int status = RPO_JPEG_OK;
  for (int u = 0; u < f.units; ++u) status = std::max(status, decode_unit(file, nbytes, d, tab, coef, u, rst[u]));
  pixels(coef, f, tab->quant, rgb);
  free(coef);
  return status;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3 && argc != 4) {
    fprintf(stderr, "usage: %s IN OUT [probe]\n", argv[0]);
    return 2;
  }
  const bool probe_only = argc == 4;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int32_t n = 0;
  if (fread(&n, 4, 1, in) != 1) return 2;
  for (int k = 0; k < n; ++k) {
    int64_t nbytes = 0;
    if (fread(&nbytes, 8, 1, in) != 1 || nbytes <= 0) return 2;
    uint8_t* file = static_cast<uint8_t*>(malloc((size_t)nbytes));              // 16-byte aligned, exactly nbytes
    if (!file || fread(file, 1, (size_t)nbytes, in) != (size_t)nbytes) return 2;
    rpo_jpeg_info f;
    int32_t rec[12] = {rpo_jpeg_prog_probe(file, nbytes, &f), -1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1};
    std::vector<uint8_t> rgb;
    if (rec[0] == 0 && !probe_only) {
      void* blob = aligned_alloc(16, (size_t)f.table_bytes);
      if (!blob || rpo_jpeg_prog_plan(file, nbytes, blob, f.table_bytes) != 0 || !prog_info_consistent(f)) return 3;
      if (rpo_jpeg_prog_plan(file, nbytes, blob, f.table_bytes - 1) != RPO_E_WORKSPACE) return 3;
      rgb.resize((size_t)f.width * f.height * 3);
      rec[1] = decode_progressive(file, nbytes, f, static_cast<const ProgHead*>(blob), rgb.data());
      free(blob);
    } else if (rec[0] == RPO_E_JPEG_SEQUENTIAL && !probe_only) {
      rec[11] = rpo_jpeg_probe(file, nbytes, &f);
      if (rec[11] == 0) {
        Tables* tab = static_cast<Tables*>(aligned_alloc(16, sizeof(Tables)));
        if (!tab || rpo_jpeg_tables(file, nbytes, tab, sizeof(Tables)) != 0 || !info_consistent(f)) return 3;
        rgb.resize((size_t)f.width * f.height * 3);
        rec[1] = decode_baseline(file, nbytes, f, tab, rgb.data());
        free(tab);
      }
    }
    if (rec[0] == 0 || rec[11] == 0) {
      const int32_t v[9] = {f.width, f.height, f.components, f.h_samp, f.v_samp, f.reserved, f.units, (int32_t)f.scan_offset,
                            (int32_t)f.table_bytes};
      memcpy(rec + 2, v, sizeof(v));
    }
    fwrite(rec, 4, 12, out);
    if (!rgb.empty()) fwrite(rgb.data(), 1, rgb.size(), out);
    free(file);
  }
  fclose(in);
  if (fclose(out) != 0) return 2;
  printf("%s %d files\n", probe_only ? "probed" : "decoded", n);
  return 0;
}
