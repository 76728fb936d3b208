"""GPU: `ovn_deskew` (csrc/deskew.hip, include/ovn_hip_deskew.h) against its float64 reference
(tests/_deskew_ref.py), its exactness promises, the azimuth time source, a bent scan of the test scene brought back onto its hits, and
every refusal of the header.

The bound.  Per coordinate |kernel - reference| <= k 2^-24 (|p| + |tau| |v|), with k counted to first order from the header's operation
sequence.  U = 2^-24, P = |p|, V = |tau| |v|; assumed: sinf within 2 ulp (a relative 4 U), |a| <= 0.5 (asserted for the inputs).
  a = tau th: tau's subtraction, th's rounding, the product: 3 U |a|.    sa: 3 U |a| + 4 U |a| = 7 U |a|.
  sh = sinf(a / 2): 3.5 U |a|;  c1 = (2 sh) sh <= a^2 / 2: relative 2 * 7 U + U = 15 U, absolute 7.5 U a^2.
  kp = cross(k, p): k's components carry U each, each product then 2 U, |k_j p_l| + |k_l p_j| <= P, the subtraction U P: 3 U P.
  kkp: sqrt(2) * 3 U P inherited + 3 U P of its own = 7.25 U P.
  sa kp: 7 U |a| P + |a| 3 U P + U |a| P = 11 U |a| P.    c1 kkp: (7.5 + 3.625 + 0.5) U a^2 P = 11.625 U a^2 P.
  the two additions of r: U (1 + |a|) P + U (1 + |a| + a^2 / 2) P.          r: U P (2 + 13 |a| + 12.125 a^2)
  B = c1 / a (<= |a| / 2): relative 15 U + 3 U + U, absolute 9.5 U |a| (the series branch has less).  B kv: 10.5 U |a| |v|.
  C = (a - sa) / a (<= a^2 / 6): the sine's 4 U |a| is absolute in the numerator: (4 U |a| + 1.67 U |a|^3) / |a| + 4 U a^2 / 6
      = 4 U + 2.34 U a^2.    C kkv: (4 + 2.67 a^2) U |v|.
  u = (v + B kv) + C kkv: v's rounding U |v|, the two additions U (2 + |a| + a^2 / 6) |v|:    u: U |v| (7 + 11.5 |a| + 2.84 a^2)
  t = tau u: + tau's U and the product's U on |u| <= (1 + |a| / 2 + a^2 / 6) |v|:              t: U V (9 + 12.5 |a| + 3.17 a^2)
  p' = r + t: U ((1 + |a| + a^2 / 2) P + (1 + |a| / 2 + a^2 / 6) V).
  Sum: P (3 + 14 |a| + 12.625 a^2) + V (10 + 13 |a| + 3.34 a^2); at |a| = 0.5 that is 13.2 P + 17.3 V: k = 17.34 (`_deskew_ref.kernel_k`).
The azimuth route adds |xi| |p| delta_s with delta_s = 4.1 * 2^-24, derived at `_deskew_ref.AZIMUTH_DELTA_S` with atan2f within 2 ulp.
The largest observed ratios to these bounds are printed and recorded in DESIGN.md section 37; k was fixed before the kernel ran."""
import ctypes as C

import numpy as np
import pytest
import torch

import _deskew_ref as DR
import _render_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

COUNTS = [0, 1, 5, 65, 513]          # scans that start in the middle of a wave (1, 6) and of a workgroup (71)
LEAD, TAIL = 3, 2                    # rows of `points` before the first scan and behind the last: never read, never written
T_REF = 0.5
A_MAX = 0.5
SENTINEL = -7.5


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


ZERO = np.zeros(6)
ZERO_SIGNED = np.array([0.0, -0.0, 0.0, -0.0, 0.0, 0.0])
TRANSLATION = np.array([2.0, -1.0, 0.3, 0.0, 0.0, 0.0])
ROTATION = np.concatenate([np.zeros(3), 0.37 * _unit([0.2, -0.3, 1.0])])
SCREW = np.concatenate([[1.5, 0.5, -0.2], 0.375 * _unit([1.0, 2.0, 3.0])])              # |a| up to 0.8 * 0.375 = 0.3
TINY = np.concatenate([[1.0, 1.0, 0.1], 1e-9 * _unit([0.0, 0.0, 1.0])])
BELOW = np.concatenate([[0.8, -0.4, 0.0], 0.9 * DR.SERIES_BELOW_F32 / 0.8 * _unit([1.0, -1.0, 2.0])])   # every |a| under the threshold
ABOVE = np.concatenate([[0.8, -0.4, 0.0], 1.1 * DR.SERIES_BELOW_F32 / 0.8 * _unit([1.0, -1.0, 2.0])])   # the outer times above it
NAN_TWIST = np.array([1.0, 0.0, 0.0, 0.0, np.nan, 0.0])
INF_TWIST = np.array([np.inf, 0.0, 0.0, 0.0, 0.0, 0.1])
TWIST_SETS = {"plain": [ZERO, ZERO_SIGNED, TRANSLATION, ROTATION, SCREW],
              "edges": [SCREW, NAN_TWIST, TINY, BELOW, ABOVE],
              "moved": [TRANSLATION, SCREW, ZERO, INF_TWIST, BELOW]}


@pytest.fixture(scope="module")
def eng():
    from overlapnet_amd.engine import OvnEngine
    e = OvnEngine(64, 900, 4, device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def batch():
    """points (LEAD + 584 + TAIL, 4), times, offsets (6,): the five scans, with the special times and values in them."""
    g = np.random.default_rng(5)
    total = LEAD + sum(COUNTS) + TAIL
    pts = np.concatenate([g.uniform(-40, 40, (total, 3)), g.uniform(0, 1, (total, 1))], 1).astype(np.float32)
    times = g.uniform(-0.2, 1.3, total).astype(np.float32)
    offsets = LEAD + np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.int64)
    pts[offsets[1], :3] = [-0.0, 3.0, -0.0]                           # the one-point scan
    for s in (2, 3, 4):
        a = int(offsets[s])
        pts[a, 0] = -0.0
        times[a + 1] = np.nan
        times[a + 2] = [np.inf, -np.inf, np.nan][s - 2]
    a = int(offsets[3])
    times[a + 3:a + 7] = [0.0, 1.0, -0.2, 1.3]
    a = int(offsets[4])
    times[a + 3:a + 8] = [0.0, 1.0, -0.2, 1.3, T_REF]
    return dict(points=pts, times=times, offsets=offsets)


def _dev(a, eng):
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def _run(eng, batch, twists, out=None, **kw):
    from overlapnet_amd.deskew import deskew_scans
    pts = _dev(batch["points"], eng)
    if out is None:
        out = torch.full_like(pts, SENTINEL)
    kw = kw or dict(times=_dev(batch["times"], eng))
    got = deskew_scans(eng, pts, _dev(batch["offsets"], eng), _dev(np.stack(twists), eng), t_ref=T_REF, out=out, **kw)
    torch.cuda.synchronize()
    return got.cpu().numpy()


def _nearest(a, b):
    """The distance of every row of a (n,3) to the nearest row of b (m,3), by differences (no squared-norm expansion)."""
    return np.concatenate([np.sqrt(((a[i:i + 256, None, :] - b[None, :, :]) ** 2).sum(-1)).min(axis=1) for i in range(0, a.shape[0], 256)])


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def results(eng, batch):
    return {name: _run(eng, batch, tw) for name, tw in TWIST_SETS.items()}


@pytest.mark.parametrize("name", sorted(TWIST_SETS))
def test_kernel_stays_within_the_counted_bound_of_the_reference(results, batch, name):
    k = DR.kernel_k(A_MAX)
    offs, got = batch["offsets"], results[name]
    worst = 0.0
    for s, xi in enumerate(TWIST_SETS[name]):
        a, b = int(offs[s]), int(offs[s + 1])
        p, t = batch["points"][a:b], batch["times"][a:b]
        want = DR.deskew(p, t, xi, T_REF)
        if b == a or not np.isfinite(xi).all():
            assert np.array_equal(_bits(got[a:b]), _bits(p))
            continue
        scale, angle = DR.bound_scale(p, t, xi, T_REF)
        assert angle.max() <= A_MAX
        err = np.abs(got[a:b, :3].astype(np.float64) - want[:, :3]).max(axis=1)
        ratio = err / (k * DR.U * scale)
        worst = max(worst, float(ratio.max()))
        assert np.all(ratio <= 1.0), (name, s, float(ratio.max()))
        assert np.array_equal(_bits(got[a:b, 3]), _bits(p[:, 3]))                           # the intensity is copied
    print("DESKEW %s: largest |kernel - reference| / (k 2^-24 (|p| + |tau||v|)) = %.3f with k = %.2f" % (name, worst, k))
    assert np.all(got[:LEAD] == SENTINEL) and np.all(got[int(offs[-1]):] == SENTINEL)         # rows outside the scans are not written
    assert worst > 0.0


def test_exact_cases(results, batch):
    offs, pts, times = batch["offsets"], batch["points"], batch["times"]
    rows = lambda s: slice(int(offs[s]), int(offs[s + 1]))
    # a zero twist (of either sign) copies the scan bit for bit, -0.0 included
    for name, s in (("plain", 1), ("moved", 2)):
        got, src = results[name][rows(s)], pts[rows(s)]
        assert np.array_equal(_bits(got), _bits(src)) and np.signbit(got[0, 0]) and got[0, 0] == 0.0
    # a twist with a non-finite entry copies it too, whatever its times
    for name, s in (("edges", 1), ("moved", 3)):
        assert np.array_equal(_bits(results[name][rows(s)]), _bits(pts[rows(s)]))
    # a point whose time is not finite becomes (0, 0, 0, intensity)
    for name, s in (("plain", 2), ("plain", 3), ("plain", 4), ("edges", 4)):
        a = int(offs[s])
        for r in (a + 1, a + 2):
            assert not np.isfinite(times[r]) and np.array_equal(results[name][r], [0.0, 0.0, 0.0, pts[r, 3]])
    # the point at tau = 0 stays where it is: r = p exactly and t = 0
    r = int(offs[4]) + 7
    assert times[r] == T_REF and np.array_equal(_bits(results["plain"][r]), _bits(pts[r]))


@pytest.mark.parametrize("name", sorted(TWIST_SETS))
def test_same_bits_in_place_again_and_alone(eng, results, batch, name):
    from overlapnet_amd.deskew import deskew_scans
    twists, offs = TWIST_SETS[name], batch["offsets"]
    a, b = int(offs[0]), int(offs[-1])
    again = _run(eng, batch, twists)
    assert np.array_equal(_bits(again), _bits(results[name]))
    pts = _dev(batch["points"], eng)
    same = deskew_scans(eng, pts, _dev(offs, eng), _dev(np.stack(twists), eng), times=_dev(batch["times"], eng), t_ref=T_REF, out=pts)
    assert same is pts
    in_place = pts.cpu().numpy()
    assert np.array_equal(_bits(in_place[a:b]), _bits(results[name][a:b]))
    assert np.array_equal(_bits(in_place[:a]), _bits(batch["points"][:a])) and np.array_equal(_bits(in_place[b:]), _bits(batch["points"][b:]))
    # each scan alone, and in a batch where it stands elsewhere (the order reversed scan by scan is not expressible with ascending
    # offsets, so: the last three scans as a batch of their own)
    for s0, s1 in [(s, s + 1) for s in range(5)] + [(2, 5)]:
        alone = _run(eng, dict(batch, offsets=offs[s0:s1 + 1]), twists[s0:s1])
        lo, hi = int(offs[s0]), int(offs[s1])
        assert np.array_equal(_bits(alone[lo:hi]), _bits(results[name][lo:hi])), (s0, s1)
        assert np.all(alone[:lo] == SENTINEL) and np.all(alone[hi:] == SENTINEL)


@pytest.mark.parametrize("start, clockwise", [(-180.0, True), (-180.0, False), (37.5, True), (37.5, False)])
def test_azimuth_route(eng, start, clockwise):
    """No point within 1e-3 rad of the seam, so every point is compared.  The bound: the kernel's, with tau from the reference's
    time, plus |xi| |p| delta_s for the float32 error of the fraction (derived for a start azimuth within -180 .. 180 degrees)."""
    g = np.random.default_rng(int(abs(start)) + int(clockwise))
    n = 700
    yaw = np.radians(start) + g.uniform(2e-3, 2 * np.pi - 2e-3, n)
    yaw[:4] = np.radians(start) + np.array([2e-3, 2 * np.pi - 2e-3, np.pi, 0.5 * np.pi])
    rng, z = g.uniform(2.0, 40.0, n), g.uniform(-3.0, 3.0, n)
    pts = np.stack([rng * np.cos(yaw), -rng * np.sin(yaw), z, g.uniform(0, 1, n)], 1).astype(np.float32)     # yaw = -atan2(y, x)
    pts[5, 0] = np.nan                                                  # no azimuth, no time: (0, 0, 0, intensity)
    seam = np.abs(np.angle(np.exp(1j * (-np.arctan2(pts[:, 1].astype(np.float64), pts[:, 0].astype(np.float64)) - np.radians(start)))))
    assert np.nanmin(seam) > 1e-3
    counts = [300, 0, 400]
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    twists = [SCREW, SCREW, np.concatenate([[-1.0, 2.0, 0.1], 0.3 * _unit([0.1, 0.1, -1.0])])]
    got = _run(eng, dict(points=pts, offsets=offs), twists, start_azimuth=start, clockwise=clockwise)
    times = DR.azimuth_times(pts, start, clockwise)
    assert np.nanmin(times) > 1e-4 and np.nanmax(times) < 1 - 1e-4 and np.isnan(times[5])
    k, worst = DR.kernel_k(A_MAX), 0.0
    for s, xi in enumerate(twists):
        a, b = int(offs[s]), int(offs[s + 1])
        if a == b:
            continue
        want = DR.deskew(pts[a:b], times[a:b], xi, T_REF)
        scale, angle = DR.bound_scale(pts[a:b], times[a:b], xi, T_REF)
        assert angle.max() <= A_MAX
        norm = np.linalg.norm(np.nan_to_num(pts[a:b, :3].astype(np.float64)), axis=1)
        bound = k * DR.U * scale + np.linalg.norm(xi) * norm * DR.AZIMUTH_DELTA_S
        err = np.abs(got[a:b, :3].astype(np.float64) - want[:, :3]).max(axis=1)
        keep = np.isfinite(times[a:b])
        worst = max(worst, float((err[keep] / bound[keep]).max()))
        assert np.all(err[keep] <= bound[keep])
    assert np.array_equal(got[5], [0.0, 0.0, 0.0, pts[5, 3]])
    print("DESKEW azimuth start %g clockwise %s: largest error / bound = %.3f" % (start, clockwise, worst))


def test_bent_scan_lands_on_its_hits(eng):
    """The generator's bent 16 x 180 scan, deskewed with its true twist and times and projected: every occupied pixel's vertex, taken
    to the world by T_ref in float64, lies within the kernel's bound (sqrt(3) of the per-coordinate one) of a recorded hit."""
    from overlapnet_amd.deskew import deskew_scans
    pose, xi, pts, times, hits = DR.kernel_scan()
    n = pts.shape[0]
    offs = _dev(np.array([0, n], np.int64), eng)
    fixed = deskew_scans(eng, _dev(pts, eng), offs, xi[None], times=_dev(times, eng), t_ref=T_REF)
    m = eng.project(fixed, offs, n, 16, 180, R.FOV_UP, R.FOV_DOWN, R.MAX_RANGE, want=("range", "vertex"))
    rng, vtx = m["range"][0].cpu().numpy(), m["vertex"][0].cpu().numpy()
    occupied = rng > 0
    assert occupied.sum() > 0.5 * n
    v = vtx[occupied].astype(np.float64)
    v[:, 3] = 1.0
    world = (pose @ v.T).T[:, :3]
    dist = _nearest(world, hits)
    scale, angle = DR.bound_scale(pts, times, xi, T_REF)
    bound = np.sqrt(3.0) * DR.kernel_k(A_MAX) * DR.U * scale.max()
    # the same scan without the deskew is off by what the host test measured: decimetres
    raw = eng.project(_dev(pts, eng), offs, n, 16, 180, R.FOV_UP, R.FOV_DOWN, R.MAX_RANGE, want=("range", "vertex"))
    rv = raw["vertex"][0].cpu().numpy()[raw["range"][0].cpu().numpy() > 0].astype(np.float64)
    rv[:, 3] = 1.0
    # each raw point against ITS OWN hit is what is off; the nearest hit of the whole scene can be closer, so this is only reported
    raw_dist = _nearest((pose @ rv.T).T[:, :3], hits)
    print("DESKEW bent scan: %d of %d pixels occupied, farthest vertex %.3e m from a hit (bound %.3e m); undeskewed: %.3f m"
          % (occupied.sum(), rng.size, dist.max(), bound, raw_dist.max()))
    assert angle.max() <= A_MAX and dist.max() <= bound


def test_refusals_leave_the_output_untouched(eng, batch):
    lib = eng.lib
    pts, times = _dev(batch["points"], eng), _dev(batch["times"], eng)
    offs, tw = _dev(batch["offsets"], eng), _dev(np.stack(TWIST_SETS["plain"]), eng)
    out = torch.full_like(pts, SENTINEL)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    base = dict(ctx=eng._h, stream=eng._stream(), points=p(pts), offsets=p(offs), n=5, times=p(times), start=0.0, cw=0, twists=p(tw),
                t_ref=T_REF, out=p(out))
    call = lambda **kw: lib.ovn_deskew(*[dict(base, **kw)[k] for k in ("ctx", "stream", "points", "offsets", "n", "times", "start", "cw",
                                                                         "twists", "t_ref", "out")])
    off = lambda t, b: C.c_void_p(t.data_ptr() + b)
    refused = [("ctx is NULL", dict(ctx=None)), ("n_scans", dict(n=-1)), ("t_ref", dict(t_ref=float("nan"))),
               ("t_ref", dict(t_ref=float("inf"))), ("t_ref", dict(t_ref=1e60)), ("start_azimuth", dict(start=float("nan"), times=None)),
               ("start_azimuth", dict(start=float("-inf"))), ("clockwise", dict(cw=2)), ("clockwise", dict(cw=-1, times=None)),
               ("NULL", dict(points=None)), ("NULL", dict(offsets=None)), ("NULL", dict(twists=None)), ("NULL", dict(out=None)),
               ("aligned", dict(points=off(pts, 4))), ("aligned", dict(out=off(out, 8)))]
    for text, kw in refused:
        assert call(**kw) == 1, kw
        assert text.encode() in lib.ovn_last_error(), (kw, lib.ovn_last_error())
    assert call(n=0, points=None, offsets=None, twists=None, out=None) == 0          # no scans: a no-op, whatever the pointers
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out[LEAD:LEAD + sum(COUNTS)] != SENTINEL).any())
