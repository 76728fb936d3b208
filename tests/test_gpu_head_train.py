"""GPU (MI355X): the weight gradients of the Delta head (`ovn_delta_head_grad`, csrc/delta_head_backward.hip) and the trainer on top
of them (overlapnet_amd/train.py) against the fp64 restatement of tests/_head_grad_ref.py.

Geometries (W, s): (45, 15) G = 3, H = 1: every dO2 position has one tap; (60, 15) G = 4: overlapping taps; (77, 15) R = 75 < W:
dropped rows get no gradient and K = R G is no multiple of 16; (50, 16) and (45, 10): s != 15; (360, 15): the real tile counts,
two pairs.  Pair counts 1, 3 and OVN_GRAD_PAIR_BLOCK + 1 (crosses the ordered reduction; run again in chunks of one pair block),
index lists with repeats and the 1-vs-N form, both losses.

Per case
  1. the signs of the returned o2 / o3 equal the fp64 reference's except on units whose fp64 pre-activation lies within the fp32
     kernels' elementwise error bound (oracle.error_bounds.head_bounds, 'generic') of zero -- at most 0.1 % of a tensor (the host
     guard holds the fixtures to that); the GPU's masks are then forced into the reference;
  2. every gradient tensor stays within 4 T of fp64, T = max |g32 - g64| of the same restatement in float32 on the CPU with the same
     masks (both are fp32 sums of the same terms in other orders; a dropped tap, a transposed layout or an unmasked unit is
     10^3 x larger); overlap within oracle.error_bounds.overlap_bound of the logit bound, the loss within scale x the loss's
     largest slope x the mean of those bounds (+ 4 u |loss| for its own fp32 sum);
  3. the same call twice, and the call cut into chunks of one pair block, give the same bits.
With OVN_HEAD_TRAIN_PARITY_JSON set, the measured ratios max |g_gpu - g64| / T per tensor and case are written to that file
(profiles/head_train_parity.json is such a run)."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import error_bounds as E
from tests import _head_grad_ref as R
from tools import synthetic as S

pytestmark = pytest.mark.gpu

_RATIOS = {}


def _engine(W, s, weights, **model_extra):
    from overlapnet_amd.engine import OvnEngine
    h, wi = R.GEOMS[(W, s)]
    e = OvnEngine(h, wi, 4)
    try:
        e.load_weights(weights, dict(R.model_cfg(W, s), **model_extra))
        assert e.feat_w == W and e.conv1size == s
    except Exception:
        e.close()
        raise
    return e


@pytest.fixture(scope="module")
def parity_file():
    yield
    path = os.environ.get("OVN_HEAD_TRAIN_PARITY_JSON")
    if path and _RATIOS:
        worst = max(max(v.values()) for v in _RATIOS.values())
        with open(path, "w") as f:
            json.dump({"what": "max |g_gpu - g64| / max |g32_cpu - g64| per gradient tensor (pass: <= 4)", "worst": worst,
                       "cases": _RATIOS}, f, indent=1, sort_keys=True)


def _call(eng, c, **kw):
    dev = eng.device
    pool, right = torch.from_numpy(c["pool"]).to(dev), torch.from_numpy(c["right"]).to(dev)
    return eng.delta_head_grad(pool, right, c["targets"], lidx=c["lidx"], ridx=c["ridx"], loss=c["loss"], **kw)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_gradients_against_fp64(case, parity_file):
    W, s, n, form, loss = case
    c, ref = R.reference(case)
    eng = _engine(W, s, c["weights"])
    try:
        assert eng.head_param_sizes() == [128 * s * 64, 64, s * 64 * 128, 128, 9 * 128 * 256, 256, (W // s - 2) ** 2 * 256, 1]
        out = _call(eng, c, want_activations=True)
        again = _call(eng, c, want_activations=True)
        chunked = None
        if n > R.PAIR_BLOCK:
            eng.set_head_pipeline(chunk_pairs=R.PAIR_BLOCK)          # two chunks: one pair block, then the rest
            chunked = _call(eng, c)
            eng.set_head_pipeline()
        got = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items() if k != "grads"}
        grads = {name: out["grads"][name.split("/")[0]][name.split("/")[1]].cpu().numpy() for name in R.HEAD_PARAMS}
        # 3. determinism and chunking
        for k in ("flat", "loss", "overlap", "o2", "o3"):
            assert torch.equal(out[k], again[k]), k
        if chunked is not None:
            for k in ("flat", "loss", "overlap"):
                assert torch.equal(out[k], chunked[k]), "chunked " + k
    finally:
        eng.close()
    # 1. same linear region
    und = R.undecided(c, ref)
    masks = []
    for k, pre in (("o2", "pre2"), ("o3", "pre3")):
        m = got[k] > 0
        differ = m != (ref[pre] > 0)
        print("%s: %d of %d signs differ, %d units undecided" % (k, differ.sum(), differ.size, und[k].sum()))
        assert not np.any(differ & ~und[k]), k
        assert und[k].mean() <= 1e-3
        masks.append(m)
    # 2. gradients on the branch the GPU took
    ref64 = R.head_loss(c["weights"], c["l"], c["r"], c["targets"], s, loss, masks=masks)
    ref32 = R.head_loss(c["weights"], c["l"], c["r"], c["targets"], s, loss, masks=masks, dtype=torch.float32)
    ratios = {}
    for name in R.HEAD_PARAMS:
        g64 = ref64["grads"][name]
        assert grads[name].shape == g64.shape, name
        T = float(np.max(np.abs(ref32["grads"][name].astype(np.float64) - g64)))
        err = float(np.max(np.abs(grads[name].astype(np.float64) - g64)))
        ratios[name] = err / T if T > 0 else (0.0 if err == 0 else float("inf"))
        print("%-24s max|g64| %.3e  T %.3e  gpu err %.3e  ratio %.3f" % (name, np.abs(g64).max(), T, err, ratios[name]))
    _RATIOS["-".join(str(v) for v in case)] = ratios
    ob = R.overlap_bounds(c, ref)
    yerr = np.abs(got["overlap"].astype(np.float64) - ref["y"])
    lbound = R.LOSS_SLOPE[loss] * float(ob.mean()) + 4 * E.U32 * abs(ref["loss"])
    lerr = abs(float(got["loss"][0]) - ref["loss"])
    print("overlap err / bound %.3f   loss err %.3e bound %.3e" % (float(np.max(yerr / ob)), lerr, lbound))
    assert np.all(yerr <= ob)
    assert lerr <= lbound
    for name in R.HEAD_PARAMS:
        assert ratios[name] <= 4.0, (name, ratios[name])


def test_argument_errors():
    from overlapnet_amd._lib import OvnError
    c = R.make_case(45, 15, 3, "idx", "mse")
    eng = _engine(45, 15, c["weights"])
    try:
        pool = torch.from_numpy(c["pool"]).to(eng.device)
        with pytest.raises(ValueError):
            eng.delta_head_grad(pool, pool, c["targets"], lidx=c["lidx"], ridx=c["ridx"], loss="hinge")
        with pytest.raises(ValueError):
            eng.delta_head_grad(pool, pool, c["targets"], lidx=c["lidx"], ridx=c["ridx"], scale=float("nan"))
        with pytest.raises(IndexError):
            eng.delta_head_grad(pool, pool, c["targets"], lidx=[0, 1, 99], ridx=c["ridx"])
        with pytest.raises(OvnError):
            eng.delta_head_grad(pool, pool, c["targets"][:2], lidx=c["lidx"], ridx=c["ridx"])
        import ctypes as C
        t = torch.zeros(3, device=eng.device)
        rc = eng.lib.ovn_delta_head_grad(eng._h, C.c_void_p(pool.data_ptr()), None, C.c_void_p(pool.data_ptr()), None, 3,
                                         C.c_void_p(t.data_ptr()), 2, 1.0, C.c_void_p(t.data_ptr()), C.c_void_p(t.data_ptr()),
                                         None, None, None, None)
        assert rc == 1 and b"loss" in eng.lib.ovn_last_error()
    finally:
        eng.close()


# ---- the trainer --------------------------------------------------------------------------------------------------------------

def _infer_cfg(W, s, root, weights_file="", **model_extra):
    return {"model": dict(R.model_cfg(W, s), **model_extra), "infer_seqs": "07", "data_root_folder": str(root), "use_depth": True,
            "use_normals": True, "use_class_probabilities": False, "use_class_probabilities_pca": False, "use_intensity": False,
            "batch_size": 8, "pretrained_weightsfilename": weights_file, "precision": "f32", "stream_ahead": False}


def test_negated_differences_through_the_trainer(tmp_path):
    """deltaLayer_negateDiffs: the library differentiates the negated kernel it holds; `gradients` / `weights()` speak of the file's."""
    from overlapnet_amd.infer import Infer
    from overlapnet_amd.train import OverlapHeadTrainer, lr_schedule
    case = (45, 15, 3, "idx", "mse")
    c = R.make_case(*case)
    inf = Infer(_infer_cfg(45, 15, tmp_path, deltaLayer_negateDiffs=True), weights=c["weights"])
    try:
        inf.feature_volumes = list(c["pool"][:, None])
        tr = OverlapHeadTrainer(inf, 1e-3, loss="mse", loss_weight=1.0)
        g = tr.gradients(c["lidx"], c["ridx"], c["targets"])
        ref64 = R.head_loss(c["weights"], c["l"], c["r"], c["targets"], 15, "mse", negate=True)
        masks = [ref64["pre2"] > 0, ref64["pre3"] > 0]
        ref32 = R.head_loss(c["weights"], c["l"], c["r"], c["targets"], 15, "mse", negate=True, masks=masks, dtype=torch.float32)
        for name in R.HEAD_PARAMS:
            g64 = ref64["grads"][name]
            T = float(np.max(np.abs(ref32["grads"][name].astype(np.float64) - g64)))
            err = float(np.max(np.abs(g[name].cpu().numpy().astype(np.float64) - g64)))
            print("%-24s T %.3e gpu err %.3e ratio %.3f" % (name, T, err, err / T))
            assert err <= 4 * T, name
        before = tr.weights()
        tr.step(c["lidx"], c["ridx"], c["targets"])
        after = tr.weights()
        lr = lr_schedule(0, 1e-3, 0.99)
        for name in R.HEAD_PARAMS:
            gf = g[name].cpu().numpy().reshape(before[name].shape)
            want = before[name] - np.float32(lr) * gf / (np.abs(gf) + np.float32(1e-7))
            assert np.allclose(after[name], want, rtol=1e-5, atol=1e-9), name
        for k in c["weights"]:                       # the legs are untouched
            if k not in R.HEAD_PARAMS:
                assert np.array_equal(after[k], c["weights"][k]), k
    finally:
        inf.close()


def test_trajectory_and_stored_file(tmp_path):
    """12 Adagrad steps follow the fp64 CPU trajectory within the loss bounds carried forward (bound_k = sum_{j <= k} own_j, own_j =
    loss_weight x 6 x the mean overlap bound of step j's batch: each step's rounding enters the parameters and stays); the loss
    falls; the saved file reloads to the same bits."""
    from overlapnet_amd.infer import Infer
    from overlapnet_amd.train import OverlapHeadTrainer
    t, x, ref = R.TRAJ, R.trajectory_inputs(), R.trajectory()
    inf = Infer(_infer_cfg(t["W"], t["s"], tmp_path), weights=x["weights"])
    path = str(tmp_path / "fitted.npz")
    try:
        inf.feature_volumes = list(x["vols"][:, None])
        tr = OverlapHeadTrainer(inf, t["lr"], t["alpha"], t["loss"], t["loss_weight"])
        losses = tr.fit(x["left"], x["right"], x["targets"], t["epochs"], t["batch"], t["seed"])
        assert len(losses) == 12 and tr.epoch == 3
        steps = ref["steps_with_equal_masks"]
        assert steps >= 6
        for k in range(steps):
            print("step %2d  gpu %.6f  fp64 %.6f  diff %.2e  bound %.2e" % (k, losses[k], ref["losses64"][k],
                                                                             abs(losses[k] - ref["losses64"][k]), ref["bound"][k]))
        for k in range(steps):
            assert abs(losses[k] - ref["losses64"][k]) <= ref["bound"][k] + 4 * E.U32 * abs(ref["losses64"][k]), k
        assert losses[-1] < losses[0]
        tr.save(path)
        feats = inf.feature_volumes.device_features
        mine = inf.engine.heads(feats, feats, lidx=x["left"], ridx=x["right"])["overlap"].cpu()
    finally:
        inf.close()
    fresh = Infer(_infer_cfg(t["W"], t["s"], tmp_path, weights_file=path))
    try:
        fresh.feature_volumes = list(x["vols"][:, None])
        feats = fresh.feature_volumes.device_features
        theirs = fresh.engine.heads(feats, feats, lidx=x["left"], ridx=x["right"])["overlap"].cpu()
    finally:
        fresh.close()
    assert torch.equal(mine, theirs)


def test_delta_cache_rows_follow_the_fitted_head(tmp_path, fixture_npz):
    """After `fit`, a 1-vs-N sweep over Delta cache rows (f16x3, 360 columns) equals the same sweep on a fresh Infer loaded from the
    saved file: the rows built under the old head have been rebuilt."""
    from overlapnet_amd.infer import Infer
    from overlapnet_amd.train import OverlapHeadTrainer
    seq = tmp_path / "data" / "07"
    for sub in ("depth", "normal"):
        os.makedirs(seq / sub)
    n = 6
    for i in range(n):
        src, shift = i % 2, 60 * (i // 2)
        np.save(seq / "depth" / ("%06d.npy" % i), np.ascontiguousarray(np.roll(fixture_npz["range_%d" % src], shift, axis=1)))
        np.save(seq / "normal" / ("%06d.npy" % i), np.ascontiguousarray(np.roll(fixture_npz["normal_%d" % src], shift, axis=1)))
    w = S.make_test_weights(4, seed=0)
    path = str(tmp_path / "fitted360.npz")

    def cfg(weights_file=""):
        c = _infer_cfg(360, 15, tmp_path / "data", weights_file=weights_file)
        c["precision"] = "f16x3"
        return c

    refs = list(range(n - 1))
    inf = Infer(cfg(), weights=w)
    try:
        inf.cache_frames(n - 1)
        assert inf.feature_volumes.device_delta_cache is not None
        stale = inf.feature_volumes.device_delta_cache.clone()
        tr = OverlapHeadTrainer(inf, 1e-3)
        tr.fit([0, 1, 2, 3], [1, 2, 3, 4], [0.9, 0.1, 0.8, 0.2], epochs=1, batch_size=4)
        assert not torch.equal(stale, inf.feature_volumes.device_delta_cache)
        tr.save(path)
        ov_a, yaw_a = inf.infer_multiple(n - 1, refs)
    finally:
        inf.close()
    fresh = Infer(cfg(path))
    try:
        fresh.cache_frames(n - 1)
        ov_b, yaw_b = fresh.infer_multiple(n - 1, refs)
    finally:
        fresh.close()
    assert np.array_equal(np.asarray(ov_a).view(np.uint32), np.asarray(ov_b).view(np.uint32))
    assert np.array_equal(yaw_a, yaw_b)
