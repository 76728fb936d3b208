"""What the semantic model's input costs from raw scans (ovn_project_semantic, include/ovn_hip.h) -> profiles/semantic_projection.json.

The 1025 clouds of bench.py's `fullstack` record (tools/synthetic.fullstack_cloud: the two tests/golden scans rotated about z) with
seeded per-point class probabilities (20 per point, generated on the device), resident in HBM.  Timed with HIP events, median of
alternating repeats in one process:
  * ovn_project, stacked C = 4 (depth | normals): the `fullstack` projection;
  * ovn_project_semantic, stacked C = 24 (+ 20 class probabilities) and C = 25 (+ intensity);
  * the host-to-device copy of the probabilities from pinned memory (one gen_semantic_data batch of 64 scans, scaled to 1025);
  * the leg at C = 24 against C = 4 (C = 4 runs the fused front kernel, any other C the generic first layer).
Bytes moved per projection: points (16 B each), the key image (8 B per pixel), the stacked output (4 C B per pixel) and, for the
semantic calls, the winners' probability rows (80 B per pixel with a point); over kernel time as a fraction of the HBM peak.
Run on one MI355X: python tools/bench_semantic_projection.py [--repeats 15] [--out profiles/semantic_projection.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import synthetic as S                      # noqa: E402
from overlapnet_amd.engine import OvnEngine           # noqa: E402

PEAK_HBM_BPS = 8.0e12       # MI355X HBM3E, spec (bench.py uses the same figure)
NC = 20


def _median_ms(fns, repeats, dev):
    """fns: name -> callable.  Each repeat runs every callable once, in turn, between its own pair of events."""
    times = {k: [] for k in fns}
    for _ in range(repeats):
        evs = []
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            evs.append((k, a, b))
        torch.cuda.synchronize(dev)
        for k, a, b in evs:
            times[k].append(a.elapsed_time(b))
    return {k: float(np.median(v)) for k, v in times.items()}, {k: [float(x) for x in v] for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=1025)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--leg-scans", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "semantic_projection.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    fx = S.load_fixture_images()
    clouds = [S.fullstack_cloud(fx, i) for i in range(args.scans)]
    counts = [c.shape[0] for c in clouds]
    offs_h = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    total = int(offs_h[-1])
    pts = torch.from_numpy(np.concatenate(clouds)).to(dev)
    offs = torch.from_numpy(offs_h).to(dev)
    del clouds
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    probs = torch.rand((total, NC), generator=g, device=dev)
    mx = max(counts)
    n, H, W = args.scans, 64, 900

    e4 = OvnEngine(H, W, 4, device=0)
    e24 = OvnEngine(H, W, 24, device=0)
    e4.load_weights(S.make_test_weights(4, seed=0), S.REFERENCE_MODEL_CFG)
    e24.load_weights(S.make_test_weights(24, seed=0), S.REFERENCE_MODEL_CFG)
    out4 = torch.empty((n, H, W, 4), dtype=torch.float32, device=dev)
    out24 = torch.empty((n, H, W, 24), dtype=torch.float32, device=dev)
    out25 = torch.empty((n, H, W, 25), dtype=torch.float32, device=dev)

    def proj4():
        e4.project(pts, offs, mx, want=(), stacked_flags=(True, True, False), stacked_out=out4)

    def proj24():
        e4.project(pts, offs, mx, want=(), stacked_flags=(True, True, True, False), stacked_out=out24, probs=probs, n_points=total)

    def proj25():
        e4.project(pts, offs, mx, want=(), stacked_flags=(True, True, True, True), stacked_out=out25, probs=probs, n_points=total)

    # correctness of what is timed: the cue channels of the semantic calls are ovn_project's
    for f in (proj4, proj24, proj25):
        f()
    torch.cuda.synchronize(dev)
    assert torch.equal(out24[..., :4], out4) and torch.equal(out25[..., :4], out4)
    filled = int((out24[..., 4] >= 0).sum().item())          # pixels with a point under max_range = inf
    cue_px = int((out4[..., 0] >= 0).sum().item())

    proj_ms, proj_all = _median_ms({"ovn_project_c4": proj4, "semantic_c24": proj24, "semantic_c25": proj25}, args.repeats, dev)

    # host-to-device copy of one gen_semantic_data batch (64 scans) of probabilities from pinned memory
    b_rows = int(offs_h[min(64, n)])
    host = torch.empty((b_rows, NC), dtype=torch.float32, pin_memory=True)
    host.copy_(probs[:b_rows].cpu())
    dst = torch.empty((b_rows, NC), dtype=torch.float32, device=dev)
    h2d_ms, h2d_all = _median_ms({"h2d_64_scans": lambda: dst.copy_(host, non_blocking=True)}, args.repeats, dev)

    # leg at C = 24 against C = 4 on the projected inputs
    L = min(args.leg_scans, n)
    fv = torch.empty((L, 360, 128), dtype=torch.float32, device=dev)
    x4, x24 = out4[:L].contiguous(), out24[:L].contiguous()
    e4.leg(x4, out=fv)
    e24.leg(x24, out=fv)
    leg_ms, leg_all = _median_ms({"leg_c4": lambda: e4.leg(x4, out=fv), "leg_c24": lambda: e24.leg(x24, out=fv)}, args.repeats, dev)

    hw = n * H * W
    bytes_c4 = 16.0 * total + hw * (8 + 4 * 4)
    bytes_sem = {c: 16.0 * total + hw * (8 + 4 * c) + filled * 4 * NC for c in (24, 25)}
    gb = lambda b: b / 1e9
    rec = {
        "what": "ovn_project (stacked C=4) vs ovn_project_semantic (C=24 / 25) on bench.py's fullstack clouds; H2D of the "
                "probabilities; leg at C=24 vs C=4",
        "device": torch.cuda.get_device_name(dev),
        "scans": n, "points": total, "max_points": mx, "pixels": hw, "pixels_with_point_inf": filled, "pixels_with_cue_point": cue_px,
        "repeats": args.repeats, "timing": "HIP events around each call, median of alternating repeats in one process",
        "ms": {**proj_ms, **h2d_ms, **leg_ms},
        "gather_extra_ms": {"c24": proj_ms["semantic_c24"] - proj_ms["ovn_project_c4"],
                            "c25": proj_ms["semantic_c25"] - proj_ms["ovn_project_c4"]},
        "bytes_gb": {"ovn_project_c4": gb(bytes_c4), "semantic_c24": gb(bytes_sem[24]), "semantic_c25": gb(bytes_sem[25]),
                     "h2d_64_scans": gb(b_rows * NC * 4.0)},
        "frac_of_hbm_peak": {"ovn_project_c4": bytes_c4 / (proj_ms["ovn_project_c4"] * 1e-3) / PEAK_HBM_BPS,
                             "semantic_c24": bytes_sem[24] / (proj_ms["semantic_c24"] * 1e-3) / PEAK_HBM_BPS,
                             "semantic_c25": bytes_sem[25] / (proj_ms["semantic_c25"] * 1e-3) / PEAK_HBM_BPS},
        "h2d_gb_per_s": b_rows * NC * 4.0 / (h2d_ms["h2d_64_scans"] * 1e-3) / 1e9,
        "h2d_ms_per_1025_scans": h2d_ms["h2d_64_scans"] * total / b_rows * 1025 / n,
        "leg_scans": L,
        "leg_ms_per_scan": {"c4": leg_ms["leg_c4"] / L, "c24": leg_ms["leg_c24"] / L},
        "all_ms": {**proj_all, **h2d_all, **leg_all},
        "peak_hbm_bps": PEAK_HBM_BPS,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: rec[k] for k in ("ms", "gather_extra_ms", "frac_of_hbm_peak", "h2d_gb_per_s", "h2d_ms_per_1025_scans",
                                          "leg_ms_per_scan")}))
    e4.close()
    e24.close()


if __name__ == "__main__":
    main()
