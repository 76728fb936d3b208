"""GPU (MI355X): the semantic model's input from raw scans -- ovn_project_semantic (class probabilities projected beside the cues in
one launch sequence, gen_semantic_data.py:33-46) and `Infer` with config['scan_folder'] + config['semantic_folder'] against the .npy
route on the files the demo1 drivers and gen_semantic_data write from the same scans."""
import os
import shutil

import numpy as np
import pytest
import torch

from oracle import overlapnet_oracle as O
from tools import synthetic as S

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]


def _clouds(fx):
    """Clouds of different sizes in one batch, with points beyond 50 m (a whole sector of one cloud only beyond it), zero-depth and
    NaN points ahead of winners, duplicated points (ties) and an empty scan."""
    rng = np.random.default_rng(5)
    a = fx["points_0"].astype(np.float32).copy()
    yaw = np.arctan2(a[:, 1], a[:, 0])
    far = (yaw > 0.3) & (yaw < 0.7)                      # this sector's pixels hold only points beyond 50 m
    a[far, :3] *= np.float32(6.0)
    bad = np.zeros((400, 4), np.float32)
    bad[200:, :3] = np.nan
    bad[:, 3] = 0.5
    a = np.insert(a, rng.integers(0, a.shape[0], 400), bad, axis=0)   # scattered ahead of many winners
    a = np.concatenate([bad[:7], a])                     # ... and ahead of every point
    b = S.transformed_cloud(fx, 13)[::3].copy()
    dup = rng.integers(0, b.shape[0], 5000)
    b = np.concatenate([b, b[dup]])                      # exact duplicates: equal keys but for the index
    c = fx["points_1"][rng.permutation(fx["points_1"].shape[0])[:50000]].astype(np.float32)
    return [a, np.zeros((0, 4), np.float32), b, c]


def _batch(eng, clouds, nc=20, seed=11):
    rng = np.random.default_rng(seed)
    probs = [rng.random((c.shape[0], nc)).astype(np.float32) for c in clouds]
    counts = [c.shape[0] for c in clouds]
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    pts = torch.from_numpy(np.concatenate(clouds)).to(eng.device)
    pr = torch.from_numpy(np.concatenate(probs)).to(eng.device)
    return pts, torch.from_numpy(offs).to(eng.device), max(counts), probs, pr, offs


@pytest.fixture(scope="module")
def eng():
    from overlapnet_amd.engine import OvnEngine
    e = OvnEngine(64, 900, 4, device=0)
    yield e
    e.close()


CUES = ("range", "vertex", "intensity", "idx", "normal")


def test_cue_view_is_ovn_project(eng, fixture_npz):
    pts, off, mx, probs, pr, _ = _batch(eng, _clouds(fixture_npz))
    for ui in (False, True):
        plain = eng.project(pts, off, mx, max_range=50, want=CUES, stacked_flags=(True, True, ui))
        sem = eng.project(pts, off, mx, max_range=50, want=CUES, stacked_flags=(True, True, True, ui), probs=pr)
        for k in CUES:
            assert torch.equal(plain[k], sem[k]), k
        cue_ch = [0, 1, 2, 3] + ([24] if ui else [])
        assert sem["stacked"].shape[-1] == (25 if ui else 24)
        assert torch.equal(sem["stacked"][..., cue_ch], plain["stacked"])
    # the fixture cases are really there: pixels with points only beyond 50 m, an empty scan
    inf = eng.project(pts, off, mx, max_range=np.inf, want=("range",))["range"]
    only_far = (inf > 0) & (plain["range"] < 0)
    assert int(only_far[0].sum()) > 500 and bool((inf[1] == -1).all())


def test_semantic_view_takes_the_reference_rows(eng, fixture_npz):
    clouds = _clouds(fixture_npz)
    pts, off, mx, probs, pr, _ = _batch(eng, clouds)
    idx = eng.project(pts, off, mx, max_range=np.inf, want=("idx",))["idx"]
    r = eng.project(pts, off, mx, max_range=50, want=("semantic", "sem_idx"), probs=pr)
    assert torch.equal(r["sem_idx"], idx)
    idx = idx.cpu().numpy()
    sem = r["semantic"].cpu().numpy()
    for s, c in enumerate(clouds):
        want = np.full((64, 900, 20), -1, np.float32)
        m = idx[s] >= 0
        want[m] = probs[s][idx[s][m]]
        assert np.array_equal(sem[s], want), s
    # the shifted-row rule is exercised: scan 0's winners sit behind zero-depth / NaN points, so proj_idx is not the winner's row
    a = clouds[0]
    d = np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
    kept = np.flatnonzero((d > 0) & (d < np.inf))
    m = idx[0] >= 0
    unshifted = probs[0][kept[idx[0][m]]]
    assert not np.array_equal(sem[0][m], unshifted)


@pytest.mark.parametrize("ui", [False, True])
def test_stacked_is_depth_normals_probabilities_intensity(eng, fixture_npz, ui):
    pts, off, mx, probs, pr, offs = _batch(eng, _clouds(fixture_npz))
    r = eng.project(pts, off, mx, want=("range", "normal", "intensity", "semantic"), stacked_flags=(True, True, True, ui), probs=pr)
    parts = [r["range"][..., None], r["normal"], r["semantic"]] + ([r["intensity"][..., None]] if ui else [])
    assert torch.equal(r["stacked"], torch.cat(parts, dim=-1))
    # probability rows only 4-byte aligned: the generic kernel, same bits
    buf = torch.empty(pr.numel() + 1, dtype=torch.float32, device=eng.device)
    buf[1:].copy_(pr.view(-1))
    odd = buf[1:].view(pr.shape)
    assert odd.data_ptr() % 16 == 4
    r2 = eng.project(pts, off, mx, want=("semantic",), stacked_flags=(True, True, True, ui), probs=odd, n_points=int(offs[-1]))
    assert torch.equal(r2["stacked"], r["stacked"]) and torch.equal(r2["semantic"], r["semantic"])


def test_other_class_counts(eng, fixture_npz):
    from overlapnet_amd._lib import OvnError
    clouds = _clouds(fixture_npz)
    pts, off, mx, probs, pr, _ = _batch(eng, clouds, nc=7, seed=3)
    r = eng.project(pts, off, mx, want=("range", "normal", "intensity", "semantic", "sem_idx"),
                    stacked_flags=(True, True, True, True), probs=pr, n_classes=7)
    idx = eng.project(pts, off, mx, max_range=np.inf, want=("idx",))["idx"]
    assert torch.equal(r["sem_idx"], idx)
    idx = idx.cpu().numpy()
    sem = r["semantic"].cpu().numpy()
    for s in range(len(clouds)):
        want = np.full((64, 900, 7), -1, np.float32)
        m = idx[s] >= 0
        want[m] = probs[s][idx[s][m]]
        assert np.array_equal(sem[s], want), s
    parts = [r["range"][..., None], r["normal"], r["semantic"], r["intensity"][..., None]]
    assert torch.equal(r["stacked"], torch.cat(parts, dim=-1)) and r["stacked"].shape[-1] == 12
    for nc in (0, 65):
        with pytest.raises(OvnError):
            eng.project(pts, off, mx, want=("semantic",), probs=torch.zeros((pr.shape[0], max(nc, 1)), device=eng.device),
                        n_classes=nc)
    with pytest.raises(OvnError):       # one row per point
        eng.project(pts, off, mx, want=("semantic",), probs=pr[1:].contiguous(), n_classes=7)


# ---- Infer ------------------------------------------------------------------------------------------------------------------------
def _write_frames(tmp_path, fx, n, intensity):
    """Raw scans + .label files, and the .npy files the demo1 drivers and gen_semantic_data write from them."""
    from overlapnet_amd import preprocess as P
    scans, labels, seq = tmp_path / "scans", tmp_path / "labels", tmp_path / "data" / "07"
    for d in (scans, labels, seq, tmp_path / "sem"):
        os.makedirs(d)
    clouds = [S.transformed_cloud(fx, i) for i in range(n)]
    probs = []
    for i, c in enumerate(clouds):
        c.tofile(scans / ("%06d.bin" % i))
        p = np.random.default_rng(200 + i).random((c.shape[0], 20)).astype(np.float32)
        p.tofile(labels / ("%06d.label" % i))
        probs.append(p)
    P.gen_depth_data(str(scans), str(seq))
    P.gen_normal_data(str(scans), str(seq))
    if intensity:
        P.gen_intensity_data(str(scans), str(seq))
    P.gen_semantic_data(str(labels), str(scans), str(tmp_path / "sem"))
    shutil.copytree(tmp_path / "sem" / "semantic", seq / "probability")
    return scans, labels, clouds, probs


def _config(tmp_path, intensity, **extra):
    cfg = {"model": dict(S.REFERENCE_MODEL_CFG, inputShape=[64, 900]), "infer_seqs": "07", "data_root_folder": str(tmp_path / "data"),
           "use_depth": True, "use_normals": True, "use_class_probabilities": True, "use_class_probabilities_pca": False,
           "use_intensity": intensity, "batch_size": 4, "pretrained_weightsfilename": ""}
    cfg.update(extra)
    return cfg


def test_infer_semantic_model_from_raw_scans(tmp_path, fixture_npz):
    from overlapnet_amd.infer import Infer
    n = 6
    scans, labels, clouds, probs = _write_frames(tmp_path, fixture_npz, n, intensity=False)
    w = S.make_test_weights(24, seed=0)
    a = Infer(_config(tmp_path, False, scan_folder=str(scans), semantic_folder=str(labels)), weights=w)
    b = Infer(_config(tmp_path, False), weights=w)
    assert a.no_input_channels == 24
    for i in range(n):
        ra, rb = a.infer_multiple(i, list(range(i))), b.infer_multiple(i, list(range(i)))
        assert (ra is None and rb is None) or (np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1])), i
        if i == 3:
            assert a._ahead_fv == "000004"              # frame 4's projection + leg ran on the look-ahead context ...
    assert a._qa is not None and a._ahead_fv is None    # ... and was adopted; there is no frame 6 to read ahead
    assert torch.equal(a.feature_volumes.device_features, b.feature_volumes.device_features)
    oa, ya = a.infer_one(str(scans / "000001.bin"), str(scans / "000004.bin"))
    ob, yb = b.infer_one(str(scans / "000001.bin"), str(scans / "000004.bin"))
    assert np.array_equal(oa, ob) and np.array_equal(ya, yb)
    assert np.array_equal(a.create_feature_volumes(["000002", "000005"]), b.create_feature_volumes(["000002", "000005"]))
    assert a.infer_top_k(n - 1, list(range(n - 1)), k=3, overlap_thres=None) == \
        b.infer_top_k(n - 1, list(range(n - 1)), k=3, overlap_thres=None)
    ca = Infer(_config(tmp_path, False, scan_folder=str(scans), semantic_folder=str(labels)), weights=w)
    cb = Infer(_config(tmp_path, False), weights=w)
    ca.cache_frames(n)
    cb.cache_frames(n)
    assert torch.equal(ca.feature_volumes.device_features, cb.feature_volumes.device_features)
    qs, lists = [5, 3, 4], [[0, 1, 2], [0, 1, 2, 4], [5, 0]]
    assert ca.infer_top_k_batch(qs, lists, k=2, overlap_thres=None) == cb.infer_top_k_batch(qs, lists, k=2, overlap_thres=None)
    # runtime errors, raised before any kernel runs
    os.remove(labels / "000002.label")
    with pytest.raises(Exception, match="Could not read semantic file .*000002.label"):
        a.create_feature_volumes(["000002"])
    probs[3][:-1].tofile(labels / "000003.label")
    with pytest.raises(Exception, match="000003.label") as ei:
        a.create_feature_volumes(["000003"])
    assert ("%d rows" % (clouds[3].shape[0] - 1)) in str(ei.value) and ("%d points" % clouds[3].shape[0]) in str(ei.value)
    for o in (a, b, ca, cb):
        o.close()


def test_infer_semantic_c25_against_the_fp64_oracle(tmp_path, fixture_npz):
    from overlapnet_amd.infer import Infer
    scans, labels, clouds, probs = _write_frames(tmp_path, fixture_npz, 2, intensity=True)
    w = S.make_test_weights(25, seed=1)
    a = Infer(_config(tmp_path, True, scan_folder=str(scans), semantic_folder=str(labels)), weights=w)
    b = Infer(_config(tmp_path, True), weights=w)
    oa, ya = a.infer_one(str(scans / "000000.bin"), str(scans / "000001.bin"))
    ob, yb = b.infer_one(str(scans / "000000.bin"), str(scans / "000001.bin"))
    assert np.array_equal(oa, ob) and np.array_equal(ya, yb)
    imgs = []
    for i in (1, 0):                 # l = frame 1 (second argument), r = frame 0 (infer.py:140,150-152)
        rng, vtx, inten, _ = O.range_projection(clouds[i])
        _, _, _, idx = O.range_projection(clouds[i], max_range=np.inf)
        sem = np.full((64, 900, 20), -1, np.float32)
        sem[idx >= 0] = probs[i][idx[idx >= 0]]
        imgs.append(np.concatenate([rng[..., None], O.gen_normal_map(rng, vtx), sem, inten[..., None]], axis=-1).astype(np.float32))
    o_ov, o_yaw, _, _, _ = O.infer_pairs(np.stack(imgs), np.array([[0, 1]]), w, S.REFERENCE_MODEL_CFG, np.float64)
    assert abs(float(oa[0]) - float(o_ov[0])) <= 1e-4 and int(ya[0]) == int(o_yaw[0])
    a.close()
    b.close()
