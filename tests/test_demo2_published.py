"""GPU: the demo1 + demo2 flow of the reference (tools/demo2_published.py: the two shipped scans -> depth / normal .npy files ->
`Infer(config).infer_one(scan2_path, scan1_path)` with config/network.yml as shipped) on a full-size Keras-layout weight file with
SEEDED weights, against the fp64 oracle.  The pin on the published demo2 result itself needs the authors' trained model_geo.weight,
which is not in this tree: `python tools/demo2_published.py /path/to/model_geo.weight` runs it."""
import os

import numpy as np
import pytest
import torch

from tools.demo2_published import run_demo2

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]


def test_demo2_flow_on_a_keras_layout_file_with_seeded_weights(tmp_path, fixture_npz):
    """The same demo1 + demo2 flow, always run: a full-size Keras-layout HDF5 file written by real h5py with SEEDED weights
    (tests/golden/make_keras_full_golden.py) stands in for model_geo.weight; expected values come from the fp64 oracle with the
    roles of infer.py:138-152 (scan1 = file 000000 -> head left, scan2 = 000001 -> head right)."""
    _check_seeded_flow(tmp_path, fixture_npz, None)


def test_demo2_flow_on_a_keras_layout_file_with_seeded_weights_fp32(tmp_path, fixture_npz):
    """The same, with every contraction on the fp32 matrix cores (the `precision` key)."""
    _check_seeded_flow(tmp_path, fixture_npz, "f32")


def _check_seeded_flow(tmp_path, fixture_npz, precision):
    from oracle import overlapnet_oracle as O
    from tools import synthetic as S
    from overlapnet_amd import weights as W
    wfile = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keras_layout_full_c4.weight")
    _, overlap, yaw = run_demo2(tmp_path, fixture_npz, wfile, precision)
    w = W.load_weights_file(wfile)
    imgs = np.stack([S.stack(fixture_npz["range_%d" % i], fixture_npz["normal_%d" % i], None, (True, True, False)) for i in range(2)])
    fv = O.leg_forward(imgs, w, S.REFERENCE_MODEL_CFG, np.float64)
    o_ov, o_yaw, _, _ = O.heads_forward(fv[[0]], fv[[1]], w)
    assert abs(float(overlap[0]) - o_ov[0]) <= 1e-4 and int(yaw[0]) == int(o_yaw[0])
