"""`ovn_icp_register` (csrc/icp_register.hip) timed with HIP events at 64 x 900 and 20 iterations, for 5 pairs (a top-5 verification)
and for 1024 pairs against one target, next to a batched torch-on-GPU restatement of the same passes -- what a user would write
without the kernel: per-point arithmetic fp32, sums fp64 (bmm), batched Cholesky, no host synchronisation inside the loop, the 1024
pairs in chunks of `--torch-chunk` so that the intermediates fit comfortably.

Inputs: the two fixture scans and 30 moved copies of them projected on the GPU (32 distinct scans); the 1024-pair case replicates
their maps to 1024 distinct scan slots, so every pair streams its own 1.8 MB source, and registers each onto scan 0.  Per size:
`--warmup` untimed calls of each implementation, then `reps` back-to-back calls between two events, alternating the two for
`--rounds` rounds; the per-call time is the median over the rounds.  The poses of the two implementations are compared once.
Output: ONE JSON object on stdout.

    python tools/bench_icp.py > profiles/icp_register.json"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 64, 900
FOV_UP, FOV_DOWN, MAX_RANGE = 3.0, -25.0, 50.0
PARAMS = dict(iterations=20, max_dist=2.0, cos_min=0.8, huber=0.2, min_inliers=64)


def _time(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def _se3_exp(xi):
    v, w = xi[:, :3], xi[:, 3:]
    th2 = (w * w).sum(1)
    th = th2.sqrt()
    small = th < 1e-4
    ths = torch.where(small, torch.ones_like(th), th)
    a = torch.where(small, 1.0 - th2 / 6.0, torch.sin(ths) / ths)
    b = torch.where(small, 0.5 - th2 / 24.0, (1.0 - torch.cos(ths)) / (ths * ths))
    c = torch.where(small, 1.0 / 6.0 - th2 / 120.0, (ths - torch.sin(ths)) / (ths * ths * ths))
    z = torch.zeros_like(th)
    K = torch.stack([z, -w[:, 2], w[:, 1], w[:, 2], z, -w[:, 0], -w[:, 1], w[:, 0], z], 1).reshape(-1, 3, 3)
    K2 = K @ K
    eye = torch.eye(3, dtype=xi.dtype, device=xi.device).expand_as(K)
    T = torch.zeros((xi.shape[0], 4, 4), dtype=xi.dtype, device=xi.device)
    T[:, :3, :3] = eye + a[:, None, None] * K + b[:, None, None] * K2
    T[:, :3, 3] = ((eye + b[:, None, None] * K + c[:, None, None] * K2) @ v[:, :, None])[:, :, 0]
    T[:, 3, 3] = 1.0
    return T


def torch_icp(vertex, normal, rng, src, tgt, T0, iterations=20, max_dist=2.0, cos_min=0.8, huber=0.2, min_inliers=64):
    """The passes of ovn_icp_register in batched torch ops -> (pose (P,4,4) f64, inliers (P), rms (P))."""
    P, N = src.numel(), H * W
    s = src.long()
    vs = vertex[s].reshape(P, N, 4)[..., :3]
    ns = normal[s].reshape(P, N, 3)
    src_ok = (rng[s].reshape(P, N) > 0) & ((ns * ns).sum(-1) < 1.5)
    vt, nt, rt = vertex.reshape(-1, 4), normal.reshape(-1, 3), rng.reshape(-1)
    base = tgt.long()[:, None] * N
    down = abs(FOV_DOWN) / 180.0 * math.pi
    inv_fov = 1.0 / (down + abs(FOV_UP) / 180.0 * math.pi)
    T = T0.clone()
    active = torch.ones(P, dtype=torch.bool, device=T.device)
    count = e = None
    for k in range(iterations + 1):
        R, t = T[:, :3, :3].float(), T[:, :3, 3].float()
        p = torch.baddbmm(t[:, None, :], vs, R.transpose(1, 2))
        d = p.norm(dim=2)
        yaw = -torch.atan2(p[..., 1], p[..., 0])
        pitch = torch.asin((p[..., 2] / d).clamp(-1.0, 1.0))
        uf = torch.floor(0.5 * (yaw / math.pi + 1.0) * W)
        vf = torch.floor((1.0 - (pitch + down) * inv_fov) * H)
        ok = src_ok & (d > 0) & (d < MAX_RANGE) & (vf >= 0) & (vf < H)
        pix = vf.clamp(0, H - 1).long() * W + uf.clamp(0, W - 1).long() + base
        q, n = vt[pix][..., :3], nt[pix]
        diff = p - q
        m = ns @ R.transpose(1, 2)
        ok &= (rt[pix] > 0) & ((n * n).sum(-1) < 1.5) & ((diff * diff).sum(-1) <= max_dist * max_dist) & ((n * m).sum(-1) >= cos_min)
        r = (n * diff).sum(-1)
        ar = r.abs()
        w = torch.where(ar <= huber, torch.ones_like(ar), huber / ar) * ok
        J = torch.cat([n, torch.cross(p, n, dim=-1)], -1).double()
        wJ = J * w.double()[..., None]
        rd = r.double()
        A = wJ.transpose(1, 2) @ J
        b = (wJ.transpose(1, 2) @ rd[..., None])[..., 0]
        count = ok.sum(1)
        e = (w.double() * rd * rd).sum(1)
        active = active & (count >= min_inliers)
        if k == iterations:
            break
        L, info = torch.linalg.cholesky_ex(A)
        active = active & (info == 0)
        L = torch.where(active[:, None, None], L, torch.eye(6, dtype=L.dtype, device=L.device).expand_as(L))
        xi = torch.cholesky_solve(-b[..., None], L)[..., 0]
        xi = torch.where(active[:, None], xi, torch.zeros_like(xi))
        T = _se3_exp(xi) @ T
    return T, count, (e / count.clamp(min=1)).sqrt()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch-chunk", type=int, default=128)
    ap.add_argument("--sizes", type=int, nargs="+", default=[5, 1024])
    a = ap.parse_args()
    from tools import synthetic as S
    from overlapnet_amd.engine import OvnEngine
    from overlapnet_amd import preprocess as P
    torch.cuda.set_device(0)
    eng = OvnEngine(H, W, 4, device=0)
    fx = S.load_fixture_images()
    g = np.random.default_rng(0)
    clouds, poses = [fx["points_0"], fx["points_1"]], [np.eye(4), np.eye(4)]
    for i in range(30):      # moved copies: yaw anywhere, up to 1.5 m away; the initial yaw is off by up to 0.5 degrees
        yaw, t = g.uniform(-180, 180), np.append(g.uniform(-1.5, 1.5, 2), g.uniform(-0.1, 0.1))
        c, s = math.cos(math.radians(yaw)), math.sin(math.radians(yaw))
        T = np.eye(4)
        T[:2, :2], T[:3, 3] = [[c, -s], [s, c]], t
        inv = np.linalg.inv(T)
        pts = np.array(fx["points_%d" % (i % 2)], np.float32).reshape(-1, 4).copy()
        pts[:, :3] = (pts[:, :3].astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
        clouds.append(pts)
        T0 = np.eye(4)
        o = math.radians(yaw + g.uniform(-0.5, 0.5))
        T0[:2, :2] = [[math.cos(o), -math.sin(o)], [math.sin(o), math.cos(o)]]
        poses.append(T0)
    r = P.project_scans(clouds, engine=eng, proj_H=H, proj_W=W, want=("range", "vertex", "normal"))
    rows = []
    for n_pairs in a.sizes:
        rep = max(1, -(-(n_pairs + 1) // 32))
        vertex, normal, rng = (r[k].repeat((rep,) + (1,) * (r[k].dim() - 1)).contiguous() for k in ("vertex", "normal", "range"))
        ids = np.arange(1, n_pairs + 1)                      # scan slot p + 1 onto scan 0 (slot 32 j is a copy of scan 0 itself)
        src = torch.from_numpy(ids.astype(np.int32)).cuda()
        tgt = torch.zeros(n_pairs, dtype=torch.int32, device="cuda")
        T0 = torch.from_numpy(np.stack([poses[i % 32] for i in ids])).cuda()
        hip = lambda: eng.icp_register(vertex, normal, rng, src, tgt, T0, fov_up=FOV_UP, fov_down=FOV_DOWN, max_range=MAX_RANGE, **PARAMS)
        ch = a.torch_chunk

        def tor():
            out = [torch_icp(vertex, normal, rng, src[i:i + ch], tgt[i:i + ch], T0[i:i + ch], **PARAMS) for i in range(0, n_pairs, ch)]
            return tuple(torch.cat(x) for x in zip(*out))
        hip_reps, tor_reps = (20, 3) if n_pairs <= 64 else (3, 1)
        for f in (hip, tor):
            for _ in range(a.warmup):
                f()
        torch.cuda.synchronize()
        th, tt = [], []
        for _ in range(a.rounds):
            th.append(_time(hip, hip_reps))
            tt.append(_time(tor, tor_reps))
        pose, stats = hip()
        tp, tc, trms = tor()
        dpos = (pose[:, :3, 3] - tp[:, :3, 3]).norm(dim=1)
        hm, tm = float(np.median(th)), float(np.median(tt))
        rows.append({"pairs": n_pairs, "hip_ms": round(hm, 4), "hip_ms_min": round(min(th), 4), "hip_ms_max": round(max(th), 4),
                     "torch_ms": round(tm, 3), "torch_ms_min": round(min(tt), 3), "torch_over_hip": round(tm / hm, 1),
                     "hip_us_per_pair": round(1e3 * hm / n_pairs, 2), "status_ok": int((stats[:, 0] == 0).sum()),
                     "median_inliers": float(stats[:, 2].median()),
                     "max_translation_difference_hip_vs_torch_m": float(dpos.max()),
                     "median_translation_difference_hip_vs_torch_m": float(dpos.median()),
                     "hip_reps": hip_reps, "torch_reps": tor_reps})
        del vertex, normal, rng
    eng.close()
    print(json.dumps({"tool": "tools/bench_icp.py", "device": torch.cuda.get_device_name(0), "shape": [H, W], "params": PARAMS,
                      "rounds": a.rounds, "warmup": a.warmup, "torch_chunk": a.torch_chunk,
                      "method": "HIP events around reps back-to-back calls (OvnEngine.icp_register, output allocation included; "
                                "the torch restatement in chunks of torch_chunk pairs), alternating; median per-call time over rounds",
                      "rows": rows}, indent=1))


if __name__ == "__main__":
    main()
