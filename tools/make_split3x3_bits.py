#!/usr/bin/env python3
"""SHA-256 digests of what the split 3x3 kernel writes for the cases of tests/split3x3_midstep_cases.py (run on the MI355X).

    PYTHONPATH=<built checkout of the commit to record> python tools/make_split3x3_bits.py --commit <its hash> \
        --out tests/golden/g28_split3x3_parent_bits.json

`cwfa_amd` is imported from PYTHONPATH (this checkout when it is empty); the case list and the input builder are this
checkout's, the same ones tests/test_gpu_split3x3_midstep.py runs, so the digests compare the two kernels on identical inputs.
A schedule change of the step loop keeps every accumulator's MFMAs and their order: the outputs must not move by one bit."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.append(ROOT)

import torch  # noqa: E402

import split3x3_midstep_cases as M  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit whose kernel is recorded")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    import cwfa_amd
    from cwfa_amd import ops
    print("cwfa_amd from", os.path.dirname(cwfa_amd.__file__), flush=True)
    digests = {}
    with torch.no_grad():
        for c, fmt in M.PARAMS:
            ops.set_precision(fmt)
            try:
                for variant, r in M.run_case(ops, c, fmt).items():
                    if "nodigest" not in r:
                        digests[M.key(c, fmt, variant)] = M.digest(r["y"])
            finally:
                ops.set_precision("fp32")
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"what": "SHA-256 of the output bytes of tests/split3x3_midstep_cases.py, written by tools/make_split3x3_bits.py",
                   "parent_commit": a.commit, "digests": digests}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(digests)} digests -> {a.out}")


if __name__ == "__main__":
    main()
