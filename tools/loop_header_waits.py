#!/usr/bin/env python3
"""List, per gfx950 kernel of a .hip translation unit, the inner-loop headers that open with `s_waitcnt vmcnt(0)`, and the
scratch loads / stores that sit inside inner loops (all of them, and those in loops that issue MFMAs: the GEMM loop bodies).

    python tools/loop_header_waits.py pixel-nerf_amd/csrc/pnr_split.hip [--filter eval_split] [-DMACRO ...]

Why: a register spill that hipcc reloads right in front of a GEMM loop shares the vmcnt counter with the weight ring's
requests; the loop header is one instruction for both predecessors, so it becomes `s_waitcnt vmcnt(0)` and the ring (4 k-steps of
prefetch) drains at every loop body.  tools/kernel_regs.py's spill COUNT does not show that; this does (round 6: found in a
build with 40 spills whose A/B gain had vanished; profiles/r06_split_kernel_ab.txt)."""
import re
import subprocess
import sys
import tempfile


def main():
    src = sys.argv[1]
    flt = None
    extra = []
    args = sys.argv[2:]
    while args:
        a = args.pop(0)
        if a == "--filter":
            flt = args.pop(0)
        else:
            extra.append(a)
    with tempfile.NamedTemporaryFile(suffix=".s") as f:
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "--cuda-device-only", "-S",
                        src, "-o", f.name] + extra, check=True, stderr=subprocess.DEVNULL)
        lines = open(f.name).read().split("\n")
    name, loops, bad, scr, mfma_scr = None, 0, 0, 0, 0
    out = []
    for i, ln in enumerate(lines):
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            name, loops, bad, scr, mfma_scr = m.group(1), 0, 0, 0, 0
        if "Inner Loop Header" in ln and name:
            loops += 1
            if any("vmcnt(0)" in x for x in lines[i + 1:i + 4]):
                bad += 1
            # the loop's body: from its header label to the backward branch to that label
            label = ln.split(":")[0].strip()
            body = []
            for x in lines[i + 1:]:
                body.append(x)
                if re.search(r"s_cbranch_\w+\s+" + re.escape(label) + r"\b", x) or "s_endpgm" in x:
                    break
            n_scr = sum(1 for x in body if re.match(r"\s*scratch_(load|store)", x))
            scr += n_scr
            if any("v_mfma" in x for x in body):
                mfma_scr += n_scr
        if "s_endpgm" in ln and name:
            out.append((name, loops, bad, scr, mfma_scr))
            name = None
    dem = subprocess.run(["c++filt"] + [o[0] for o in out], capture_output=True, text=True).stdout.split("\n")
    print("loops  vmcnt(0)-headers  scratch-in-inner-loops  (of which in loops with MFMAs)  kernel")
    for (n, l, b, s, ms), d in zip(out, dem):
        if flt and flt not in d:
            continue
        print(f"{l:5d}  {b:16d}  {s:22d}  {ms:30d}  {d}")


if __name__ == "__main__":
    main()
