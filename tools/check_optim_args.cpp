// Stand-alone host check of rpo_optim_step_sets' argument validation, for the host sanitizers:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         rpo_amd/csrc/optim.hip tools/check_optim_args.cpp -o /tmp/check_optim_args && /tmp/check_optim_args
//
// Every call below must be refused BEFORE any launch, so the program needs no GPU: the pointers are host memory that is
// never dereferenced.  Exit status 0 = every refusal came back with its code.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/rpo_amd.h"

static int failures = 0;
#define EXPECT(call, code)                                                                    \
  do {                                                                                        \
    const int rc_ = (call);                                                                   \
    if (rc_ != (code)) { std::printf("FAIL %s -> %d, want %d\n", #call, rc_, (code)); ++failures; } \
  } while (0)

int main() {
  std::vector<float> f(4096);
  std::vector<int32_t> i(64);
  float* p = f.data();
  int32_t* t = i.data();
  const int64_t S0 = 256, S1 = 384, ST = 1024;
  EXPECT(rpo_optim_step_sets(nullptr, p, p, p, nullptr, ST, 3, t, p, t, nullptr, S0, S1, 0, nullptr, nullptr), RPO_E_BADARG);
  EXPECT(rpo_optim_step_sets(p, nullptr, p, p, nullptr, ST, 3, t, p, t, nullptr, S0, S1, 0, nullptr, nullptr), RPO_E_BADARG);
  EXPECT(rpo_optim_step_sets(p, p, nullptr, p, nullptr, ST, 3, t, p, t, nullptr, S0, S1, 0, nullptr, nullptr), RPO_E_BADARG);
  EXPECT(rpo_optim_step_sets(p, p, p, nullptr, nullptr, ST, 3, t, p, t, nullptr, S0, S1, 0, nullptr, nullptr), RPO_E_BADARG);
  EXPECT(rpo_optim_step_sets(p, p, p, p, nullptr, ST, 3, nullptr, p, t, nullptr, S0, S1, 0, nullptr, nullptr), RPO_E_BADARG);
  EXPECT(rpo_optim_step_sets(p, p, p, p, nullptr, ST, 3, t, nullptr, t, nullptr, S0, S1, 0, nullptr, nullptr), RPO_E_BADARG);
  EXPECT(rpo_optim_step_sets(p, p, p, p, nullptr, ST, 3, t, p, nullptr, nullptr, S0, S1, 0, nullptr, nullptr), RPO_E_BADARG);
  EXPECT(rpo_optim_step_sets(p, p, p, p, nullptr, ST, 3, t, p, t, nullptr, S0, S1, 1, nullptr, nullptr), RPO_E_BADARG);  // needs_s2
  EXPECT(rpo_optim_step_sets(p, p, p, p, nullptr, ST, 0, t, p, t, nullptr, S0, S1, 0, nullptr, nullptr), RPO_E_BADARG);
  EXPECT(rpo_optim_step_sets(p, p, p, p, nullptr, ST, -1, t, p, t, nullptr, S0, S1, 0, nullptr, nullptr), RPO_E_BADARG);
  EXPECT(rpo_optim_step_sets(p, p, p, p, nullptr, ST, 3, t, p, t, nullptr, 0, 0, 0, nullptr, nullptr), RPO_E_BADARG);
  EXPECT(rpo_optim_step_sets(p, p, p, p, nullptr, ST, 3, t, p, t, nullptr, -1, S1, 0, nullptr, nullptr), RPO_E_BADARG);
  EXPECT(rpo_optim_step_sets(p, p, p, p, nullptr, ST, 3, t, p, t, nullptr, S0, -1, 0, nullptr, nullptr), RPO_E_BADARG);
  EXPECT(rpo_optim_step_sets(p, p, p, p, nullptr, S0 + S1 - 1, 3, t, p, t, nullptr, S0, S1, 0, nullptr, nullptr), RPO_E_SHAPE);
  EXPECT(rpo_optim_step_sets(p, p, p, p, nullptr, S0 + S1 - 1, 3, t, p, t, nullptr, S0, S1, 0, t, nullptr), RPO_E_SHAPE);
  EXPECT(rpo_optim_step_sets(p, p, p, p, p, ST, 65536, t, p, t, nullptr, S0, S1, 1, nullptr, nullptr), RPO_E_SHAPE);
  EXPECT(rpo_optim_step_sets(p, p, p, p, nullptr, INT64_MAX, 65536, t, p, t, t, INT64_MAX - 1, 1, 0, t, nullptr), RPO_E_SHAPE);
  EXPECT(rpo_optim_step_sets(p, p, p, p, nullptr, INT64_MAX, 3, t, p, t, nullptr, INT64_MAX, INT64_MAX, 0, nullptr, nullptr), RPO_E_SHAPE);
  std::printf(failures ? "%d refusals missing\n" : "all refusals returned their codes (%d failures)\n", failures);
  return failures != 0;
}
