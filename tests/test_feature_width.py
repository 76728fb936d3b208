"""CPU: the feature geometry of the leg for any `inputShape` (weights.feature_width) and the Infer checks that run before any GPU work.

The reference derives every shape from the input (generateNet.py:143-146, 161-214); the heads run 1 x W x 128 volumes for
45 <= W <= 512 (include/ovn_hip.h: OVN_FEAT_W_MIN / OVN_FEAT_W_MAX)."""
import numpy as np
import pytest

from overlapnet_amd import weights as W
from overlapnet_amd._lib import OvnError

A3 = {"additional_unsymmetric_layer3a": True}

# (input H, W), model keys, leg output (H_f, W_f, C)
TABLE = [
    ((64, 900), A3, (1, 360, 128)),
    ((32, 900), {}, (1, 371, 128)),
    ((16, 900), {"strides_layer1": [1, 2]}, (1, 371, 128)),
    ((64, 1024), A3, (1, 422, 128)),
    ((32, 1024), {}, (1, 433, 128)),
    ((64, 720), A3, (1, 270, 128)),
    ((64, 900), {}, (3, 371, 128)),
]


@pytest.mark.parametrize("shape,keys,out", TABLE)
def test_leg_output_shape_table(shape, keys, out):
    assert W.leg_output_shape(shape[0], shape[1], W.leg_layers(4, keys)) == out
    if out[0] == 1:
        assert W.feature_width(shape[0], shape[1], 4, keys, out[1]) == out[1]
        assert W.feature_width(shape[0], shape[1], 4, keys) == out[1]


def test_dense_shape_follows_width():
    assert W.expected_shapes(4, {}, 422)["overlap_output/kernel"] == (173056, 1)
    assert W.expected_shapes(4, {}, 422)["overlap_output/kernel"][0] == (422 // 15 - 2) ** 2 * 256
    assert W.expected_shapes(4, {})["overlap_output/kernel"] == (123904, 1)           # default unchanged
    assert W.expected_shapes(4, {"conv1NetworkHead_conv1size": 10}, 371)["overlap_output/kernel"] == (35 * 35 * 256, 1)


def test_keras_default_init_and_synthetic_weights_honour_width():
    w = W.keras_default_init(4, {}, seed=0, feat_w=371)
    assert w["overlap_output/kernel"].shape == ((371 // 15 - 2) ** 2 * 256, 1)
    assert not np.any(w["overlap_output/bias"])
    w2 = W.keras_default_init(4, {}, seed=0, feat_w=433)
    assert w2["overlap_output/kernel"].shape == (26 * 26 * 256, 1)
    assert W.keras_default_init(4, {}, seed=0)["overlap_output/kernel"].shape == (123904, 1)
    s = W.synthetic_weights(4, {}, seed=1, feat_w=270)
    assert s["overlap_output/kernel"].shape == (16 * 16 * 256, 1)
    W.check_weights(s, 4, {}, 270)
    with pytest.raises(ValueError):
        W.check_weights(s, 4, {})        # checked at 360 by default


@pytest.mark.parametrize("shape,keys,width,what", [
    ((64, 900), {}, 371, "height 1"),                                    # 3 x 371: H_f != 1
    ((32, 900), {}, 360, "leg_output_width"),                            # the key disagrees with the leg
    ((64, 1400), A3, None, "512"),                                       # W > 512
    ((64, 200), A3, None, "45"),                                         # W < 45
])
def test_feature_width_refuses(shape, keys, width, what):
    with pytest.raises(ValueError) as ei:
        W.feature_width(shape[0], shape[1], 4, keys, width)
    assert what in str(ei.value) and ("%dx%d" % shape) in str(ei.value)
    assert isinstance(ei.value, OvnError)        # ovn_finalize refused these shapes with an OvnError: callers that caught it still do


def _cfg(shape, width, **model):
    return {"model": dict({"leg_output_width": width, "inputShape": list(shape), "legsType": "360OutputkLegs",
                           "overlap_head": "DeltaLayerConv1NetworkHead", "orientation_head": "CorrelationHead"}, **model),
            "infer_seqs": "07", "data_root_folder": "/nonexistent", "use_depth": True, "use_normals": True, "use_intensity": False,
            "use_class_probabilities": False, "batch_size": 16, "pretrained_weightsfilename": ""}


@pytest.mark.parametrize("cfg,what", [
    (_cfg((64, 900), 371), "height 1"),
    (_cfg((32, 900), 360), "leg_output_width"),
    (_cfg((64, 1400), 573, additional_unsymmetric_layer3a=True), "512"),
])
def test_infer_refuses_geometry_before_any_engine(cfg, what, monkeypatch):
    from overlapnet_amd import infer as I

    def no_engine(*a, **k):
        raise AssertionError("an engine was created")

    monkeypatch.setattr(I, "OvnEngine", no_engine)
    with pytest.raises(ValueError) as ei:
        I.Infer(cfg)
    assert what in str(ei.value)


def test_infer_accepts_other_widths_up_to_the_engine(monkeypatch):
    """32 x 900 with the leg's defaults (1 x 371) passes the geometry check and reaches the engine with the right input shape."""
    from overlapnet_amd import infer as I
    seen = {}

    class Stop(Exception):
        pass

    def fake_engine(h, w, c, device=None):
        seen["shape"] = (h, w, c)
        raise Stop()

    monkeypatch.setattr(I, "OvnEngine", fake_engine)
    inf = I.Infer.__new__(I.Infer)
    with pytest.raises(Stop):
        I.Infer.__init__(inf, _cfg((32, 900), 371))
    assert seen["shape"] == (32, 900, 4) and inf.feat_w == 371


def test_sharded_infer_refuses_other_widths(monkeypatch):
    import torch.distributed as dist
    from overlapnet_amd import infer as I
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_rank", lambda group=None: 0)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    monkeypatch.setattr(I, "OvnEngine", lambda *a, **k: (_ for _ in ()).throw(AssertionError("an engine was created")))
    with pytest.raises(ValueError) as ei:
        I.Infer(_cfg((32, 900), 371), world=2)
    assert "sharded" in str(ei.value) and "371" in str(ei.value)


def test_header_documents_the_width_range():
    import os
    from overlapnet_amd import _lib
    h = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "ovn_hip.h")).read()
    assert "#define OVN_FEAT_W_MIN %d" % W.FEAT_W_MIN in h
    assert "#define OVN_FEAT_W_MAX %d" % W.FEAT_W_MAX in h
