"""Generates tests/golden/ref_icp_restatement.npz: the results of the numpy ICP restatements
(tests/icp_restatement.py, tests/depth_pyramid_restatement.py) on a fixed noisy frame pair, which
tests/test_icp_host.py::test_the_restatements_equal_their_pinned_results holds them to bit for bit.  The stored file
was written at commit df39129 ("Track ICP over a bilateral-filtered depth pyramid with a normal gate"), before the two
restatements were folded into one; it is regenerated only when the arithmetic of INTEGRATION.md section 3 changes on
purpose.  Host numpy only, a few seconds:

    python tests/golden/make_golden_icp.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from test_icp_host import pinned_runs  # noqa: E402

if __name__ == "__main__":
    runs = pinned_runs()
    for name in ("strided", "pyramid", "gated"):
        print(name, "pairs", runs[name + "_count"].tolist(),
              "rejected", runs[name + "_angle_rejected"].tolist() if name != "strided" else None)
    path = os.path.join(HERE, "ref_icp_restatement.npz")
    np.savez_compressed(path, **runs)
    print(path, os.path.getsize(path), "bytes")
