"""CPU: the checks of the raw-scan route for the semantic model (`config['semantic_folder']`) that run before any GPU work, and the
argument refusals of ovn_project_semantic that need no device."""
import os

import numpy as np
import pytest

from overlapnet_amd import _lib


def _cfg(**extra):
    cfg = {"model": {"leg_output_width": 360, "inputShape": [64, 900], "legsType": "360OutputkLegs",
                     "overlap_head": "DeltaLayerConv1NetworkHead", "orientation_head": "CorrelationHead",
                     "additional_unsymmetric_layer3a": True},
           "infer_seqs": "07", "data_root_folder": "/nonexistent", "use_depth": True, "use_normals": True, "use_intensity": False,
           "use_class_probabilities": True, "use_class_probabilities_pca": False, "batch_size": 16,
           "pretrained_weightsfilename": ""}
    cfg.update(extra)
    return cfg


class _Stop(Exception):
    pass


def _no_engine(monkeypatch):
    from overlapnet_amd import infer as I

    def no_engine(*a, **k):
        raise AssertionError("an engine was created")

    monkeypatch.setattr(I, "OvnEngine", no_engine)
    return I


@pytest.mark.parametrize("extra,err,what", [
    # the semantic model from raw scans without the probabilities: the refusal of earlier versions, text unchanged
    (dict(scan_folder="/scans"), Exception,
     "config['scan_folder']: the semantic channels come from RangeNet++ .npy files, not from the raw scans"),
    (dict(scan_folder="/scans", semantic_folder="/labels", use_class_probabilities_pca=True), ValueError, "use_class_probabilities_pca"),
    (dict(semantic_folder="/labels"), ValueError, "semantic_folder"),
    (dict(scan_folder="/scans", semantic_folder="/labels", use_class_probabilities=False), ValueError, "semantic_folder"),
])
def test_infer_refuses_semantic_configs_before_any_engine(extra, err, what, monkeypatch):
    I = _no_engine(monkeypatch)
    with pytest.raises(err) as ei:
        I.Infer(_cfg(**extra))
    assert what in str(ei.value)


@pytest.mark.parametrize("intensity,C", [(False, 24), (True, 25)])
def test_infer_takes_the_semantic_model_from_raw_scans(intensity, C, monkeypatch):
    """scan_folder + semantic_folder + use_class_probabilities reaches the engine with the semantic model's channel count."""
    from overlapnet_amd import infer as I
    seen = {}

    def fake_engine(h, w, c, device=None):
        seen["shape"] = (h, w, c)
        raise _Stop()

    monkeypatch.setattr(I, "OvnEngine", fake_engine)
    cfg = _cfg(scan_folder="/scans", semantic_folder="/labels", use_intensity=intensity)
    with pytest.raises(_Stop):
        I.Infer(cfg)
    assert seen["shape"] == (64, 900, C) and cfg["model"]["inputShape"] == [64, 900, C]


def _bare_infer(tmp_path):
    """An Infer whose engine records calls: enough state for `_inputs_from_scans` (the file checks run before any GPU work)."""
    from overlapnet_amd import infer as I

    class Recorder:
        device = "cpu"

        def project(self, *a, **k):
            raise AssertionError("the projection ran")

    inf = object.__new__(I.Infer)
    inf._scan_folder = str(tmp_path / "scans")
    inf._semantic_folder = str(tmp_path / "labels")
    inf.engine = Recorder()
    inf.inputShape = [64, 900, 24]
    inf.use_depth, inf.use_normals, inf.use_intensity = True, True, False
    os.makedirs(tmp_path / "scans")
    os.makedirs(tmp_path / "labels")
    return inf


def test_missing_and_misaligned_label_files_raise_before_the_projection(tmp_path):
    inf = _bare_infer(tmp_path)
    rng = np.random.default_rng(0)
    for i, n in enumerate((100, 37)):
        rng.random((n, 4)).astype(np.float32).tofile(tmp_path / "scans" / ("%06d.bin" % i))
    rng.random((100, 20)).astype(np.float32).tofile(tmp_path / "labels" / "000000.label")
    missing = str(tmp_path / "labels" / "000001.label")
    with pytest.raises(Exception) as ei:
        inf._inputs_from_scans(["000000", "000001"])
    assert str(ei.value) == "Could not read semantic file %s" % missing
    rng.random((36, 20)).astype(np.float32).tofile(missing)
    with pytest.raises(Exception) as ei:
        inf._inputs_from_scans(["000000", "000001"])
    msg = str(ei.value)
    assert missing in msg and "36 rows" in msg and "37 points" in msg


def test_project_semantic_refuses_bad_class_counts_and_missing_probs():
    lib = _lib.load()
    for nc in (0, 65, -1):
        rc = lib.ovn_project_semantic(None, None, None, 1, 0, 64, 900, 3.0, -25.0, 50.0, None, nc, *([None] * 8), 1, 1, 1, 0, None)
        assert rc == 1 and b"n_classes" in lib.ovn_last_error()
    # a probability output (semantic image, or the stacked input with the semantic cue) without probabilities
    rc = lib.ovn_project_semantic(None, None, None, 1, 0, 64, 900, 3.0, -25.0, 50.0, None, 20, *([None] * 5), 1, None, None,
                                  1, 1, 0, 0, None)
    assert rc == 1 and b"probs is NULL" in lib.ovn_last_error()
    rc = lib.ovn_project_semantic(None, None, None, 1, 0, 64, 900, 3.0, -25.0, 50.0, None, 20, *([None] * 7), 1, 1, 1, 1, 0, None)
    assert rc == 1 and b"probs is NULL" in lib.ovn_last_error()
    # neither: the call gets as far as the context check
    rc = lib.ovn_project_semantic(None, None, None, 1, 0, 64, 900, 3.0, -25.0, 50.0, None, 20, *([None] * 6), 1, None, 1, 1, 0, 0,
                                  None)
    assert rc == 1 and b"ctx is NULL" in lib.ovn_last_error()
