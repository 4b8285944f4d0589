#!/usr/bin/env python3
"""What stands in front of a kernel's first vector memory request, read off hipcc's assembly (no GPU needed):

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S rpo_amd/csrc/gemm_ws.hip -o ws.s
    python tools/isa_prologue.py ws.s [substring of the demangled kernel name ...]

Per kernel: instruction lines, v_rcp* and kernel-argument wait groups (an s_waitcnt on lgkmcnt with scalar loads
outstanding) in front of the first global_load / buffer_load, and the register / scratch figures of the kernel descriptor.
The count follows the textual order of the blocks, which for these kernels is the order a workgroup runs them in up to
the first request (straight-line prologues)."""
import re
import subprocess
import sys


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        return out.splitlines()
    except (OSError, subprocess.CalledProcessError):
        return list(names)


def kernels(path):
    """name -> (body lines, {metadata key: value})"""
    body, meta, cur, code = {}, {}, None, False
    for line in open(path):
        s = line.strip()
        m = re.match(r"^(_Z\w+):", line)
        if m:                                                   # a function's label; its code runs to .Lfunc_end
            cur, code = m.group(1), True
            body[cur], meta[cur] = [], {}
        elif cur is not None and s.startswith(".Lfunc_end"):
            code = False
        elif cur is not None and code:
            body[cur].append(s)
        elif cur is not None:                                   # the resource comments behind the kernel descriptor
            m = re.match(r"^; (TotalNumSgprs|NumVgprs|NumAgprs|ScratchSize): (\d+)", s)
            if m:
                meta[cur][m.group(1)] = int(m.group(2))
    return body, meta


def prologue(lines):
    n = rcp = waits = pending = 0
    for s in lines:
        if not s or s.startswith((";", ".", "//")) or s.endswith(":"):
            continue
        op = s.split()[0]
        if op.startswith(("global_load", "buffer_load", "flat_load")):
            return n, rcp, waits
        n += 1
        if op.startswith("v_rcp"):
            rcp += 1
        if op.startswith("s_load") or op.startswith("s_buffer_load"):
            pending += 1
        if op == "s_waitcnt" and "lgkmcnt" in s and pending:
            waits += 1
            pending = 0
    return n, rcp, waits


def main():
    path, wanted = sys.argv[1], sys.argv[2:]
    body, meta = kernels(path)
    names = [k for k in body if meta[k].get("NumVgprs") is not None]
    for k, d in zip(names, demangle(names)):
        if wanted and not any(w in d for w in wanted):
            continue
        n, rcp, waits = prologue(body[k])
        m = meta[k]
        print(f"{d}\n    before the first vector memory request: {n} instructions, {rcp} v_rcp, {waits} kernel-argument wait groups"
              f" | VGPR {m.get('NumVgprs')} AGPR {m.get('NumAgprs')} SGPR {m.get('TotalNumSgprs')} scratch {m.get('ScratchSize')}")


if __name__ == "__main__":
    main()
