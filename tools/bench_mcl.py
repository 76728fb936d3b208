"""One step of the overlap-based Monte Carlo localization (`overlapnet_amd.localization`, csrc/mcl.hip) timed stage by stage with HIP
events -- predict (`ovn_mcl_predict` + the read of its 16-byte record), the 1-vs-U sweep (`OvnEngine.heads` over the listed frames),
update (`ovn_mcl_update`), resample (`ovn_mcl_resample`) -- at P = 10 000 and 65 536 particles, next to a torch-on-GPU restatement of
the three new stages: what a user would write without the kernels (torch.randn noise, a gather through the grid, torch.unique for the
distinct frames -- which synchronises, as reading the record does --, fp64 sums, cumsum + searchsorted for the resampler).

The map: `--frames` moved copies of the two fixture scans on a serpentine path (2 m apart, rows 4 m apart), 1 m cells, test weights.
The particles start from `init_uniform` and stay spread over the whole map (zero odometry, 5 cm of noise), so U is close to the number
of frames: the sweep is timed at the size a global localization pays.  Per size: `--warmup` untimed calls of each stage, then `reps`
back-to-back calls between two events, alternating the HIP and the torch form for `--rounds` rounds; the per-call time is the median
over the rounds.  A whole `MonteCarloLocalizer.step` (leg of the query included, resampling forced) is timed with the host clock
around calls that end in a synchronise.  Output: ONE JSON object on stdout.

    python tools/bench_mcl.py > profiles/mcl.json"""
import argparse
import json
import math
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIGMA = (0.05, 0.05, 0.01)
ODOM = (0.0, 0.0, 0.0)


def _time(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / reps           # microseconds per call


def _moved(points, pose):
    c, s = math.cos(pose[2]), math.sin(pose[2])
    out = np.array(points, np.float32).reshape(-1, 4).copy()
    d = out[:, :2].astype(np.float64) - pose[:2]
    out[:, 0], out[:, 1] = c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1]
    return out


def torch_predict(parts, mp, cell_frame):
    p = parts.shape[0]
    z = torch.randn((p, 3), device=parts.device)
    dx, dy, dth = ODOM[0] + SIGMA[0] * z[:, 0], ODOM[1] + SIGMA[1] * z[:, 1], ODOM[2] + SIGMA[2] * z[:, 2]
    c, s = torch.cos(parts[:, 2]), torch.sin(parts[:, 2])
    parts[:, 0] += c * dx - s * dy
    parts[:, 1] += s * dx + c * dy
    parts[:, 2] = torch.remainder(parts[:, 2] + dth + math.pi, 2 * math.pi) - math.pi
    ix = torch.floor((parts[:, 0] - mp.origin_x) / mp.resolution).long()
    iy = torch.floor((parts[:, 1] - mp.origin_y) / mp.resolution).long()
    ok = (ix >= 0) & (ix < mp.nx) & (iy >= 0) & (iy < mp.ny)
    pf = torch.where(ok, cell_frame[(iy.clamp(0, mp.ny - 1) * mp.nx + ix.clamp(0, mp.nx - 1))], torch.full_like(ix, -1))
    lst = torch.unique(pf[pf >= 0])                   # sorted; its length is known to the host only after a synchronise
    slot = torch.full((mp.n_frames,), -1, dtype=torch.long, device=parts.device)
    slot[lst] = torch.arange(lst.numel(), device=parts.device)
    return pf, slot, lst


def torch_update(parts, pf, slot, frame_yaw, overlap, yaw, sigma_yaw, eps, o_min):
    on = pf >= 0
    s = slot[pf.clamp(min=0)]
    o = torch.nan_to_num(overlap[s.clamp(min=0)], nan=o_min).clamp(min=o_min)
    d = (parts[:, 2] - frame_yaw[pf.clamp(min=0)]) * (180.0 / math.pi) - yaw[s.clamp(min=0)].float()
    d = d - 360.0 * torch.round(d / 360.0)
    g = eps + (1.0 - eps) * torch.exp(-0.5 * (d / sigma_yaw) ** 2)
    prod = torch.where(on, parts[:, 3] * o * g, parts[:, 3] * (o_min * eps))
    _, e = torch.frexp(prod.max())
    w = torch.ldexp(prod, -e)
    parts[:, 3] = w
    wd = w.double()
    sw = wd.sum()
    th = parts[:, 2].double()
    return torch.stack([sw, sw * sw / (wd * wd).sum(), (wd * parts[:, 0].double()).sum() / sw, (wd * parts[:, 1].double()).sum() / sw,
                        torch.atan2((wd * torch.sin(th)).sum(), (wd * torch.cos(th)).sum()), torch.argmax(w).double(), on.sum().double()])


def torch_resample(parts, n_out):
    q = torch.floor(parts[:, 3].clamp(min=0).double() * 2.0 ** 30).long()
    C = torch.cumsum(q, 0)
    S = C[-1]
    r = torch.randint(0, 2 ** 62, (1,), device=parts.device) % S.clamp(min=1)
    anc = torch.searchsorted(C * n_out, torch.arange(n_out, device=parts.device) * S + r, right=True).clamp(max=parts.shape[0] - 1)
    out = parts[anc]
    out[:, 3] = 1.0
    return out, anc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--sizes", type=int, nargs="+", default=[10000, 65536])
    a = ap.parse_args()
    from tools import synthetic as S
    from overlapnet_amd.infer import Infer
    from overlapnet_amd.localization import MonteCarloLocalizer, OverlapMap, _features_of
    torch.cuda.set_device(0)
    fx = S.load_fixture_images()
    cfg = {"model": dict(S.REFERENCE_MODEL_CFG, inputShape=[64, 900]), "infer_seqs": "00", "data_root_folder": tempfile.gettempdir(),
           "use_depth": True, "use_normals": True, "use_class_probabilities": False, "use_class_probabilities_pca": False,
           "use_intensity": False, "batch_size": 16, "pretrained_weightsfilename": ""}
    infer = Infer(cfg, weights=S.make_test_weights(4, seed=0))
    eng = infer.engine
    g = np.random.default_rng(0)
    per_row = 32
    poses = np.array([[2.0 * (k % per_row if (k // per_row) % 2 == 0 else per_row - 1 - k % per_row), 4.0 * (k // per_row),
                       g.uniform(-math.pi, math.pi)] for k in range(a.frames)])
    clouds = [_moved(fx["points_%d" % (k % 2)], poses[k]) for k in range(a.frames)]
    mp = OverlapMap(infer, None, poses, resolution=1.0, scans=clouds)
    cache = infer.feature_volumes
    query = clouds[a.frames // 2]
    q = _features_of(infer, query)
    spec = eng.spectrum(q)
    stream = torch.cuda.current_stream()
    reps = 20
    rows = []
    for P in a.sizes:
        loc = MonteCarloLocalizer(mp, P, seed=1, resample_fraction=1.0)
        parts = loc.particles.clone()
        tparts = parts.clone()
        state = {}

        def hip_predict():
            state["pf"], state["slot"], state["lst"], _ = eng.mcl_predict(parts, ODOM, SIGMA, 1, 0, mp.cell_frame, (mp.origin_x, mp.origin_y),
                                                                          mp.resolution, mp.nx, mp.ny, mp.n_frames, record=loc._rec[0])
            stream.synchronize()
            state["u"] = int(loc._rec_np[0, 0])

        def tor_predict():
            state["tpf"], state["tslot"], state["tlst"] = torch_predict(tparts, mp, mp.cell_frame)
            state["tu"] = int(state["tlst"].numel())

        def sweep():
            u = state["u"]
            state["r"] = eng.heads(cache.device_features, q, lidx=state["lst"][:u], n=u, spec_l=cache.device_spectra, spec_r=spec,
                                   dcache_l=cache.device_delta_cache)

        def hip_update():
            state["est"] = eng.mcl_update(parts, state["pf"], state["slot"], mp.frame_yaw, state["r"]["overlap"], state["r"]["yaw"],
                                          loc.sigma_yaw, loc.eps_yaw, loc.overlap_min)

        def tor_update():
            state["test"] = torch_update(tparts, state["tpf"].long(), state["tslot"], mp.frame_yaw, state["tr"]["overlap"],
                                         state["tr"]["yaw"], loc.sigma_yaw, loc.eps_yaw, loc.overlap_min)

        out_buf = torch.empty_like(parts)

        def hip_resample():
            eng.mcl_resample(parts, 1, 0, out=out_buf, ancestors=loc._anc[:P], record=loc._rec[1])

        def tor_resample():
            state["tout"] = torch_resample(tparts, P)

        hip_predict()
        tor_predict()
        sweep()
        stages = [("predict", hip_predict, tor_predict), ("sweep", sweep, None), ("update", hip_update, tor_update),
                  ("resample", hip_resample, tor_resample)]
        row = {"particles": P, "frames": a.frames}
        for name, hip, tor in stages:
            for f in (hip, tor):
                if f is not None:
                    for _ in range(a.warmup):
                        f()
            torch.cuda.synchronize()
            th, tt = [], []
            n = 5 if name == "sweep" else reps
            for _ in range(a.rounds):
                parts[:, 3] = 1.0
                tparts[:, 3] = 1.0
                th.append(_time(hip, n))
                if tor is not None:
                    tt.append(_time(tor, n))
            row["hip_%s_us" % name] = round(float(np.median(th)), 2)
            row["hip_%s_us_min_max" % name] = [round(min(th), 2), round(max(th), 2)]
            if tor is not None:
                row["torch_%s_us" % name] = round(float(np.median(tt)), 1)
                row["torch_over_hip_%s" % name] = round(float(np.median(tt)) / float(np.median(th)), 1)
            if name == "predict":
                row["U"], row["U_torch"] = state["u"], state["tu"]
                row["off_map"] = int(loc._rec_np[0, 1])
                # the torch form's own sweep result, for the frames ITS last predict listed
                state["tr"] = eng.heads(cache.device_features, q, lidx=state["tlst"].int(), n=state["tu"], spec_l=cache.device_spectra,
                                        spec_r=spec, dcache_l=cache.device_delta_cache)
        est = state["est"].cpu().numpy()
        row["n_eff"] = round(float(est[2]), 1)
        # the whole step through the class: leg of the query + spectrum + the four stages + the estimate's copy, resampling forced
        for _ in range(a.warmup):
            loc.step(query, ODOM, SIGMA)
        torch.cuda.synchronize()
        ts, us = [], []
        for _ in range(a.rounds * 5):
            loc.init_uniform()                      # spread over the map again: every timed step scores the same kind of list
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e = loc.step(query, ODOM, SIGMA)
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
            us.append(e.frames_scored)
        row["step_ms"] = round(float(np.median(ts)), 3)
        row["step_ms_min_max"] = [round(min(ts), 3), round(max(ts), 3)]
        row["step_U_median"] = int(np.median(us))
        row["new_kernels_share_of_step"] = round(1e-3 * (row["hip_predict_us"] + row["hip_update_us"] + row["hip_resample_us"]) / row["step_ms"], 3)
        rows.append(row)
    print(json.dumps({"tool": "tools/bench_mcl.py", "device": torch.cuda.get_device_name(0), "frames": a.frames, "rounds": a.rounds,
                      "warmup": a.warmup, "reps": reps, "sigma": SIGMA,
                      "method": "HIP events around reps back-to-back calls of one stage (OvnEngine.mcl_predict + stream synchronise for "
                                "the record; OvnEngine.heads over frame_list[:U], 5 reps; OvnEngine.mcl_update; OvnEngine.mcl_resample), "
                                "alternating with the torch restatement of the same stage; median per-call time over rounds, in "
                                "microseconds.  step_ms: host clock around MonteCarloLocalizer.step + synchronise, median of 5 x rounds "
                                "calls, resampling forced (resample_fraction 1), test weights",
                      "rows": rows}, indent=1))
    infer.close()


if __name__ == "__main__":
    main()
