#!/usr/bin/env python3
"""Records the bits of rpo_attn_readonly_fwd_rows / rpo_attn_readonly_bwd at N <= 288 with a GIVEN library:

    RPO_HIP_LIB=/path/to/librpo_hip.so python tools/capture_attn_bits.py [out.json]

Run once with a library built from the commit before the long-sequence kernels, on the device type the suite runs on:
tests/test_gpu_attn_long.py then holds every later library to these hashes (tests/golden/attn_parent_bits.json) -- the
dispatch below 289 tokens must keep launching the kernels it launched, bit for bit."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main() -> None:
    import torch
    import test_gpu_attn_long as T
    out = sys.argv[1] if len(sys.argv) > 1 else T.PARENT_BITS
    bits = {f"{mode}_N{N}_B{B}_H{H}_K{Kp}": T.short_bits(mode, N, B, H, Kp)
            for mode in T.MODES for (N, B, H, Kp) in T.PARENT_CASES}
    rec = dict(device=torch.cuda.get_device_name(0), library=os.environ.get("RPO_HIP_LIB", "in-tree"), bits=bits)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump(rec, open(out, "w"), indent=1)
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
