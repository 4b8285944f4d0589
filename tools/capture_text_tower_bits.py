#!/usr/bin/env python3
"""Records the bits of the plain text tower -- the text-attention ops, CoOp / CoCoOp train steps and the forward-only
users of the block loop -- with a GIVEN tree and library:

    RPO_HIP_LIB=DIR/rpo_amd/librpo_hip.so python tools/capture_text_tower_bits.py --tree DIR [--out out.json]

`DIR` goes in front of sys.path, so `rpo_amd` is that tree's Python and library; the cases and their inputs are this tree's
tests/test_gpu_text_tower_bits.py, which uses only surface the parent commit has.  Run twice, in separate processes, with
the commit before the text tower was folded into one block loop, on the device type the suite runs on: cases whose hashes
agree go to tests/golden/text_tower_parent_bits.json (`--merge a.json b.json`), and the test holds every later tree to them."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=REPO, help="the tree whose rpo_amd is imported")
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge", nargs=2, metavar=("A", "B"), help="write the cases on which two captures agree")
    args = ap.parse_args()
    if args.merge:
        a, b = (json.load(open(f)) for f in args.merge)
        assert a["device"] == b["device"]
        same = {k: v for k, v in a["bits"].items() if b["bits"].get(k) == v}
        unstable = sorted((set(a["bits"]) | set(b["bits"])) - set(same))
        rec = dict(device=a["device"], library=a["library"], bits=same)
        print(f"{len(same)} stable cases; unstable: {unstable}")
    else:
        sys.path.insert(0, os.path.join(REPO, "tests"))
        sys.path.insert(0, os.path.abspath(args.tree))
        import torch
        import rpo_amd
        import test_gpu_text_tower_bits as T
        assert os.path.abspath(os.path.dirname(os.path.dirname(rpo_amd.__file__))) == os.path.abspath(args.tree)
        rec = dict(device=torch.cuda.get_device_name(0), library="RPO_HIP_LIB" if os.environ.get("RPO_HIP_LIB") else "in-tree",
                   bits={case: T.bits(case) for case in T.CASES})
    out = args.out or os.path.join(REPO, "tests", "golden", "text_tower_parent_bits.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump(rec, open(out, "w"), indent=1)
    if not args.merge:
        print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
