"""Generates tests/golden/hahog_adversarial.npz: what the REFERENCE's features::hahog -- compiled from the reference checkout into
oracle/_ref/libhahog_ref.so (oracle.hahog_ref) -- returns for every case of tests/hahog_cases.py.  Recorded results only, and hashes
rather than descriptors: per case and target the row count, the float32 angle column (compared within the stated 1e-4 degrees), SHA-256
of points[:, :3] and of the float32 descriptors; for the cases that go through features.extract_features_hahog the same for the image that
function forms from grey levels, with one descriptor hash per (feature_root, hahog_normalize_to_uchar).  The images themselves are
regenerated from their seeds by tests/hahog_cases.py.  Run where the reference is available; the .npz travels with the repository, so
that tests/test_gpu_hahog_adversarial.py needs no reference."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import hahog_cases as hc  # noqa: E402

rec = hc.all_records()
assert rec is not None, "oracle/_ref/libhahog_ref.so is not available"
out = os.path.join(HERE, "hahog_adversarial.npz")
np.savez_compressed(out, **rec)
for cid in hc.CASE_IDS:
    print("%-22s %6d rows" % (cid, int(rec[cid + "/n"])))
print(os.path.getsize(out), "bytes")
