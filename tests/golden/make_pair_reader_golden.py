#!/usr/bin/env python3
"""Generate tests/golden/pair_reader.npz by RUNNING the reference's own ground-truth pair reader,
`overlap_orientation_npz_file2string_string_nparray` of src/two_heads (imported unmodified, shuffle=False), on the two files
tests/test_host_logic.py::test_pair_reader_both_layouts_and_test_run writes: the demo4 layout (`overlaps` + `seq`) and the old
single-array layout, seven pairs each from `np.random.default_rng(3)`.  The inputs are stored beside the outputs so that the test
can check it still writes the same files.

Run in the build container only (needs the reference tree):    python tests/golden/make_pair_reader_golden.py
"""
import os
import sys
import tempfile

import numpy as np

REF = os.environ.get("OVERLAPNET_REFERENCE", "/root/reference")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pair_reader.npz")


def pair_arrays():
    """The test's inputs: (n x 4 float64 [f1, f2, overlap, yaw], n x 2 object array of sequence names)."""
    rng = np.random.default_rng(3)
    n = 7
    arr = np.zeros((n, 4))
    arr[:, 0] = 5
    arr[:, 1] = rng.permutation(n)
    arr[:, 2] = rng.random(n)
    arr[:, 3] = rng.integers(0, 360, n)
    seq = np.empty((n, 2), dtype=object)
    seq[:] = "07"
    return arr, seq


def main():
    sys.path.insert(0, os.path.join(REF, "src", "two_heads"))
    from overlap_orientation_npz_file2string_string_nparray import overlap_orientation_npz_file2string_string_nparray as ref
    arr, seq = pair_arrays()
    with tempfile.TemporaryDirectory() as d:
        new, old = os.path.join(d, "gt.npz"), os.path.join(d, "old.npz")
        np.savez_compressed(new, overlaps=arr, seq=seq)
        np.savez(old, arr)
        r = ref([new, old], shuffle=False)
    np.savez(OUT, input=arr, imgf1=np.array(r[0], dtype=str), imgf2=np.array(r[1], dtype=str), dir1=np.array(r[2], dtype=str),
             dir2=np.array(r[3], dtype=str), overlap=np.asarray(r[4], np.float64), orientation=np.asarray(r[5], np.float64))
    print("wrote", OUT)


if __name__ == "__main__":
    main()
