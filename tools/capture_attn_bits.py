#!/usr/bin/env python3
"""Records bits of the image tower's attention ops with a GIVEN library:

    RPO_HIP_LIB=/path/to/librpo_hip.so python tools/capture_attn_bits.py [out.json]
    RPO_HIP_LIB=/path/to/librpo_hip.so python tools/capture_attn_bits.py --image [out.json]
    python tools/capture_attn_bits.py --merge a.json b.json [out.json]

Without --image: rpo_attn_readonly_fwd_rows / rpo_attn_readonly_bwd at N <= 288.  Run once with a library built from the
commit before the long-sequence kernels, on the device type the suite runs on: tests/test_gpu_attn_long.py then holds every
later library to these hashes (tests/golden/attn_parent_bits.json) -- the dispatch below 289 tokens must keep launching the
kernels it launched, bit for bit.

--image: the cases of tests/test_gpu_image_attn_bits.py (every forward kernel of csrc/attn_image.hip at the shapes where
its code takes another path, and the backward entry points).  Run twice, in separate processes, with a library built from
the commit before the forward kernels were folded onto shared helpers; --merge writes the cases on which the two captures
agree to tests/golden/image_attn_parent_bits.json, and the test holds every later library to them."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main() -> None:
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--merge" in sys.argv:
        a, b = (json.load(open(f)) for f in args[:2])
        assert a["device"] == b["device"] and a["library"] == b["library"]
        same = {k: v for k, v in a["bits"].items() if b["bits"].get(k) == v}
        print(f"{len(same)} stable cases; unstable: {sorted((set(a['bits']) | set(b['bits'])) - set(same))}")
        rec = dict(device=a["device"], library=a["library"], bits=same)
        out = args[2] if len(args) > 2 else os.path.join(REPO, "tests", "golden", "image_attn_parent_bits.json")
    else:
        import torch
        if "--image" in sys.argv:
            import test_gpu_image_attn_bits as T
            bits = {case: T.bits(case) for case in T.CASES}
        else:
            import test_gpu_attn_long as T
            bits = {f"{mode}_N{N}_B{B}_H{H}_K{Kp}": T.short_bits(mode, N, B, H, Kp)
                    for mode in T.MODES for (N, B, H, Kp) in T.PARENT_CASES}
        out = args[0] if args else T.PARENT_BITS
        rec = dict(device=torch.cuda.get_device_name(0), library="RPO_HIP_LIB" if os.environ.get("RPO_HIP_LIB") else "in-tree",
                   bits=bits)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump(rec, open(out, "w"), indent=1)
    if "--merge" not in sys.argv:
        print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
