"""NumPy statement of the Monte Carlo localization stages of csrc/mcl.hip ("Localization"): Philox4x32-10, the motion
update, the cell lookup, the distinct-frame list, the observation model with its estimate, and the integer systematic resampler.

`arith` selects the per-particle arithmetic: np.float64 is the reference the GPU is held against; np.float32 restates the kernel
operation for operation (the kernels are compiled without FMA contraction), and its distance from the fp64 run on a test's inputs is
the figure the GPU tolerance is derived from (ten times it, the rule of tests/test_gpu_icp.py).  The lookup is float32 only: the
cell a position falls into is compared exactly."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)

KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (broadcastable), key: two -> (..., 4) uint32."""
    c = [np.asarray(v, np.uint64) & MASK for v in np.broadcast_arrays(*counter)]
    k0, k1 = np.uint64(key[0]) & MASK, np.uint64(key[1]) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & MASK, p1 & MASK, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & MASK, p0 & MASK]
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return np.stack(c, axis=-1).astype(np.uint32)


def motion_words(P, seed, step):
    """The draw of particle i: counter (i, step lo, step hi, 0), key (seed lo, seed hi) -> (P, 4) uint32."""
    return philox4x32_10((np.arange(P, dtype=np.uint64), step & 0xFFFFFFFF, (step >> 32) & 0xFFFFFFFF, 0),
                         (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))


def resample_offset_words(seed, step):
    return philox4x32_10((0, step & 0xFFFFFFFF, (step >> 32) & 0xFFFFFFFF, 1), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))


def uniform(words, arith):
    """u = ((k >> 8) + 0.5) 2^-24, each operation in `arith` (float32 rounds the sum to nearest even above 2^23, as the GPU does)."""
    return ((words >> np.uint32(8)).astype(arith) + arith(0.5)) * arith(2.0 ** -24)


def wrap_pi(t, arith):
    """Into (-pi, pi] with the kernel's float32 constants."""
    pi, two_pi, inv = arith(np.float32(np.pi)), arith(np.float32(2 * np.pi)), arith(np.float32(1 / (2 * np.pi)))
    t = t - two_pi * np.rint(t * inv)
    t = np.where(t <= -pi, t + two_pi, t)
    return np.where(t > pi, t - two_pi, t)


def predict(particles, words, odom, sigma, arith=np.float64):
    """particles (P,4) float32, words (P,4) uint32 -> the moved (P,4) in `arith` (w untouched).  The host doubles are rounded to
    float32 first, as the library does."""
    p = np.asarray(particles, np.float32).astype(arith)
    dx, dy, dth = (arith(np.float32(v)) for v in odom)
    sx, sy, sth = (arith(np.float32(v)) for v in sigma)
    u = uniform(words, arith)
    two_pi = arith(np.float32(2 * np.pi))
    rad_xy, ang_xy = np.sqrt(arith(-2.0) * np.log(u[:, 0])), two_pi * u[:, 1]
    rad_t, ang_t = np.sqrt(arith(-2.0) * np.log(u[:, 2])), two_pi * u[:, 3]
    zx, zy, zt = rad_xy * np.cos(ang_xy), rad_xy * np.sin(ang_xy), rad_t * np.cos(ang_t)
    ex, ey, eth = dx + sx * zx, dy + sy * zy, dth + sth * zt
    c, s = np.cos(p[:, 2]), np.sin(p[:, 2])
    out = p.copy()
    out[:, 0] = p[:, 0] + (c * ex - s * ey)
    out[:, 1] = p[:, 1] + (s * ex + c * ey)
    out[:, 2] = wrap_pi(p[:, 2] + eth, arith)
    return out


def angle_diff(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return d - 2 * np.pi * np.rint(d / (2 * np.pi))


def lookup(x, y, cell_frame, origin_x, origin_y, resolution, nx, ny, M, cell_offset=0):
    """float32, operation for operation: the frame of every position, -1 off the grid / non-finite / empty cell / entry >= M.
    cell_offset: `cell_frame` holds the cells from flat index cell_offset on (a far block of a grid too large for the host); a
    position on the grid whose cell lies outside that block is an error.  0 with the whole grid is the statement itself."""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    inv = np.float32(1.0 / float(resolution))
    with np.errstate(invalid="ignore", over="ignore"):
        fx = np.floor((x - np.float32(origin_x)) * inv)
        fy = np.floor((y - np.float32(origin_y)) * inv)
        ok = (fx >= 0) & (fx < np.float32(2147483648.0)) & (fy >= 0) & (fy < np.float32(2147483648.0))
        ix, iy = np.where(ok, fx, 0).astype(np.int64), np.where(ok, fy, 0).astype(np.int64)
    ok &= (ix < nx) & (iy < ny)
    cells = np.asarray(cell_frame)
    flat = np.where(ok, iy * nx + ix - int(cell_offset), 0)
    if np.any(flat < 0) or np.any(flat >= cells.size):
        raise IndexError("a position's cell lies outside the block of cells given (cell_offset %d, %d cells)" % (cell_offset, cells.size))
    f = np.where(ok, cells[flat], -1)
    return np.where((f < 0) | (f >= M), -1, f).astype(np.int32)


def distinct(particle_frame, M):
    """-> (frame_list (U) ascending, frame_slot (M), record (4))."""
    pf = np.asarray(particle_frame)
    lst = np.unique(pf[pf >= 0]).astype(np.int32)
    slot = np.full(M, -1, np.int32)
    slot[lst] = np.arange(len(lst), dtype=np.int32)
    return lst, slot, np.array([len(lst), int((pf < 0).sum()), 0, 1], np.int32)


def products(particles, particle_frame, frame_slot, frame_yaw, overlap, yaw, sigma_yaw, eps_yaw, overlap_min, arith=np.float64):
    """The unscaled weights w o g of every particle, in `arith`."""
    p = np.asarray(particles, np.float32).astype(arith)
    pf = np.asarray(particle_frame)
    M = len(frame_slot)
    U = 0 if overlap is None else len(overlap)
    ok = (pf >= 0) & (pf < M)
    slot = np.where(ok, np.asarray(frame_slot)[np.where(ok, pf, 0)], -1)
    slot = np.where(slot >= U, -1, slot)
    on = slot >= 0
    sig, eps, omin = arith(np.float32(sigma_yaw)), arith(np.float32(eps_yaw)), arith(np.float32(overlap_min))
    one_m = arith(np.float32(1.0) - np.float32(eps_yaw))
    prod = (p[:, 3] * omin) * eps
    if on.any():
        s = slot[on]
        of = np.asarray(overlap, np.float32)[s].astype(arith)
        with np.errstate(invalid="ignore"):
            o = np.where(of > omin, of, omin)
        d = (p[on, 2] - np.asarray(frame_yaw, np.float32)[pf[on]].astype(arith)) * arith(np.float32(180.0 / np.pi)) \
            - np.asarray(yaw)[s].astype(arith)
        d = d - arith(360.0) * np.rint(d / arith(360.0))
        t = d / sig
        g = eps + one_m * np.exp(arith(-0.5) * (t * t))
        prod = prod.copy()
        prod[on] = (p[on, 3] * o) * g
    return prod, on


def rescale(prod):
    """-> (weights, status): 2^-e times the products, e the frexp exponent of the largest finite positive product; status 1 and the
    products as they are when there is none."""
    prod = np.asarray(prod)
    fin = np.isfinite(prod) & (prod > 0)
    if not fin.any():
        return prod.copy(), 1
    _, e = np.frexp(prod[fin].max())
    return np.ldexp(prod, -int(e)), 0


def estimate(particles, on_map, status=0):
    """The eight doubles (+ the spread) from the particles as they are (weights already scaled), fp64."""
    p = np.asarray(particles, np.float64)
    n_on = float(np.count_nonzero(on_map))
    if status:
        return np.array([1.0, 0, 0, 0, 0, 0, -1.0, n_on]), 0.0
    w = p[:, 3]
    sw = w.sum()
    xm, ym = (w * p[:, 0]).sum() / sw, (w * p[:, 1]).sum() / sw
    wf = np.where(np.isnan(w), -np.inf, w)
    e = np.array([0.0, sw, sw * sw / (w * w).sum(), xm, ym, np.arctan2((w * np.sin(p[:, 2])).sum(), (w * np.cos(p[:, 2])).sum()),
                  float(np.argmax(wf)), n_on])
    return e, float(np.sqrt((w * ((p[:, 0] - xm) ** 2 + (p[:, 1] - ym) ** 2)).sum() / sw))


# ---- the inputs of the GPU comparisons (tests/test_gpu_mcl.py) and their float32 figures (tests/test_mcl_host.py) -----------------
PREDICT_SIZES = (1, 63, 64, 65, 1024, 1025, 65536)
PREDICT_ODOM, PREDICT_SIGMA = (0.8, -0.1, 0.05), (0.1, 0.05, 0.02)
PREDICT_SEED, PREDICT_STEP = 0xC0FFEE12345, (1 << 32) | 9
UPDATE_SIZES = (1, 65, 1025, 65536)
UPDATE_FRAMES = 37
UPDATE_OBS = dict(sigma_yaw=10.0, eps_yaw=0.01, overlap_min=0.05)
# this file in float32 against itself in fp64 on those inputs, rounded up (measured: 2.04e-6 m, 1.43e-7 rad; scaled weights 1.14e-6)
F32_PREDICT = (2.1e-6, 1.5e-7)
F32_WEIGHT = 1.2e-6


def predict_case(P):
    """(P,4) float32 particles within 50 m of the origin, any heading."""
    g = np.random.default_rng(1000 + P)
    p = np.empty((P, 4), np.float32)
    p[:, 0], p[:, 1] = g.uniform(-50, 50, P), g.uniform(-50, 50, P)
    p[:, 2] = -g.uniform(-np.pi, np.pi, P)
    p[:, 3] = g.uniform(0.1, 1.0, P)
    return p


def predict_error(got, want):
    """(largest position difference [m], largest heading difference [rad], on the circle) between two (P,4) particle sets."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got[:, :2] - want[:, :2]).max()), float(np.abs(angle_diff(got[:, 2], want[:, 2])).max())


def update_case(P):
    """Particles, their frames (a few off the map), the distinct list, and scores with NaN and below-floor entries; headings are
    concentrated (resultant length >= 0.1) and every product stays above 2^-100."""
    g = np.random.default_rng(2000 + P)
    M = UPDATE_FRAMES
    p = np.empty((P, 4), np.float32)
    p[:, 0], p[:, 1] = g.uniform(-30, 30, P), g.uniform(-30, 30, P)
    p[:, 2] = wrap_pi(g.normal(0.5, 0.8, P), np.float64)
    p[:, 3] = g.uniform(0.1, 1.0, P)
    pf = g.integers(-1, M, P).astype(np.int32)
    if P > 2:
        pf[1] = -1
    lst, slot, _ = distinct(pf, M)
    U = len(lst)
    overlap = g.uniform(0.02, 0.9, U).astype(np.float32)
    overlap[::5] = np.nan
    yaw = g.integers(-179, 181, U).astype(np.int32)
    frame_yaw = g.uniform(-np.pi, np.pi, M).astype(np.float32)
    return dict(particles=p, particle_frame=pf, frame_slot=slot, frame_yaw=frame_yaw, overlap=overlap, yaw=yaw)


def update_weights(case, arith):
    prod, on = products(case["particles"], case["particle_frame"], case["frame_slot"], case["frame_yaw"], case["overlap"], case["yaw"],
                        arith=arith, **UPDATE_OBS)
    w, status = rescale(prod)
    return w, on, status


def quanta(weights):
    """q_i = floor(w_i 2^30) as int64: 0 for negative / non-finite weights, 2^30 - 1 for weights >= 1."""
    w = np.asarray(weights, np.float32)
    with np.errstate(invalid="ignore"):
        good = (w > 0) & (w < np.inf)
        q = np.where(good & (w < 1), np.floor(np.where(good & (w < 1), w, 0).astype(np.float64) * 2.0 ** 30), 0).astype(np.int64)
    return np.where(good & (w >= 1), (1 << 30) - 1, q)


def resample(weights, n_out, words):
    """-> (ancestors (n_out) int32 or None, record (4) int32).  a_j = the smallest a with C[a] n_out > j S + r; both sides < 2^62."""
    q = quanta(weights)
    C = np.cumsum(q)
    S = int(C[-1])
    if S == 0:
        return None, np.array([1, 0, 0, 1], np.int32)
    r = (int(words[0]) | (int(words[1]) << 32)) % S
    assert S * n_out < 2 ** 62
    target = np.arange(n_out, dtype=np.int64) * S + r
    anc = np.searchsorted(C * n_out, target, side="right")
    return anc.astype(np.int32), np.array([0, n_out, 0, 1], np.int32)


def check_resample_properties(weights, n_out, anc):
    """The three properties the resampler guarantees."""
    q = quanta(weights)
    S = int(q.sum())
    assert len(anc) == n_out and np.all(np.diff(anc) >= 0), "ancestors must be non-decreasing"
    assert anc.min() >= 0 and anc.max() < len(q)
    counts = np.bincount(anc, minlength=len(q))
    assert not np.any(counts[q == 0]), "a zero-weight particle was chosen"
    # |count_i - n_out q_i / S| < 1, in integers: |count_i S - n_out q_i| < S
    assert np.all(np.abs(counts.astype(object) * S - n_out * q.astype(object)) < S), "a copy count is not within 1 of n_out q / S"
