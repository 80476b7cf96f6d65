#!/usr/bin/env python3
"""Record the bytes of the deterministic baked-volume entries (forward march, ray backward, scene march and backward, total
variation; every kind) as SHA-256 digests, for tests/test_hip_baked_bits.py.

    PIXELNERF_HIP_LIB=<library of the commit to record> PIXELNERF_ALLOW_VARIANT=1 python tools/make_baked_bits.py [out.npz [commit]]

Run it on the library of the commit whose bytes are the reference (one MI355X); the inputs are the test's own seeded arrays.
`commit`: the hash that library was built from, stored in the file as `recorded_from_commit` (the committed fixture: 760f380,
the commit before csrc/pnr_baked.hip was split, built with tools/build_objs.sh in an export of that commit).  Two runs must agree
before anything is written.  Default output: tests/golden/baked_bits.npz."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import test_hip_baked_bits as T
    from pixelnerf_amd import ops
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    dev = torch.device("cuda:0")
    a, b = T.all_digests(ops, dev), T.all_digests(ops, dev)
    differ = [k for k in a if a[k] != b[k]]
    assert not differ, f"not reproducible run to run: {differ}"
    rec = {k: np.str_(v) for k, v in a.items()}
    rec["recorded_from_commit"] = np.str_(sys.argv[2] if len(sys.argv) > 2 else "unknown")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez(out, **rec)
    print(f"wrote {out}: {len(a)} digests")


if __name__ == "__main__":
    main()
