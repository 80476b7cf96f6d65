#!/usr/bin/env python3
"""Record the bits of the fp32-class TRAINING forward (eval_ray_samples_split_train: outputs, operand images, x5, relu masks)
as SHA-256 digests, for tests/test_hip_split_shape.py::test_training_forward_bits_are_the_parent_commits.

    PIXELNERF_HIP_LIB=<library of the commit to record> PIXELNERF_ALLOW_VARIANT=1 python tools/make_split_train_bits.py [out.npz [commit]]

Run it on the library of the commit whose bits are the reference (one MI355X); the inputs are the test's own seeded samples.
`commit`: the hash that library was built from, stored in the file as `recorded_from_commit` (the committed fixture: 10072e4a821d,
the commit before the 16x16x32 core, built with tools/build_variant.sh from an export of that commit).
Default output: tests/golden/split_train_bits.npz."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import test_hip_split_shape as T
    from pixelnerf_amd import ops
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    dev = torch.device("cuda:0")
    rec = {}
    for name in T.TRAIN_BITS_SCENES:
        a, b = T.train_bits(ops, dev, name), T.train_bits(ops, dev, name)
        assert a == b, f"{name}: not reproducible run to run"
        for k, v in a.items():
            rec[f"{name}_{k}"] = np.str_(v)
    rec["recorded_from_commit"] = np.str_(sys.argv[2] if len(sys.argv) > 2 else "unknown")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez(out, **rec)
    print(f"wrote {out}: {len(rec)} digests")


if __name__ == "__main__":
    main()
