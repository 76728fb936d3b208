"""fp64 restatement of NormalizedCorrelation2D's four normalisations (NormalizedCorrelation2D.py:23-73) and the elementwise bound of
the normalised correlation vector -- test infrastructure shared by tests/test_corr_normalize.py (CPU) and
tests/test_gpu_corr_normalize.py.

A feature volume is (W, 128), W = 360 for the reference leg; Keras normalises over axis 2 of (1, 1, W, 128), the W columns, per
channel:
    none             x
    euclidean        x / sqrt(max(sum x^2, 1e-12))                        (K.l2_normalize, epsilon 1e-12)
    scaling          (x - min x) / (max x - min x + 1e-6)
    standardization  y = (x - mean x) + 1e-5,  y / sqrt(max(sum y^2, 1e-12))
The truth is the fp64 value of these formulas (not Keras' fp32 evaluation, which overflows above ~2^63 per element and loses the
+1e-5 of a large near-constant channel to the rounding of its fp32 mean).
"""
import numpy as np

from oracle import error_bounds as E

MODES = ("none", "euclidean", "scaling", "standardization")


def affine64(v, mode):
    """(m, a, s) per channel, fp64, so that x' = ((x - m) + a) s; v (..., W, 128)."""
    x = np.asarray(v, np.float64)
    zero = np.zeros(x.shape[:-2] + (1, x.shape[-1]))
    if mode == "none":
        return zero, 0.0, zero + 1.0
    if mode == "scaling":
        lo, hi = x.min(axis=-2, keepdims=True), x.max(axis=-2, keepdims=True)
        return lo, 0.0, 1.0 / ((hi - lo) + 1e-6)
    if mode == "euclidean":
        m, a = zero, 0.0
    elif mode == "standardization":
        m, a = x.mean(axis=-2, keepdims=True), 1e-5
    else:
        raise ValueError(mode)
    q = np.square((x - m) + a).sum(axis=-2, keepdims=True)
    return m, a, 1.0 / np.sqrt(np.maximum(q, 1e-12))


def normalize64(v, mode):
    """The fp64 truth of the normalised volume(s)."""
    x = np.asarray(v, np.float64)
    if mode == "scaling":      # the formula as written: a division
        lo, hi = x.min(axis=-2, keepdims=True), x.max(axis=-2, keepdims=True)
        return (x - lo) / ((hi - lo) + 1e-6)
    m, a, s = affine64(x, mode)
    return ((x - m) + a) * s


def normalize32(v, mode):
    """What the kernels store: each element evaluated in fp64 and rounded once to fp32 (csrc/ovn_internal.h)."""
    if mode == "none":
        return np.asarray(v, np.float32)
    m, a, s = affine64(v, mode)
    return (((np.asarray(v, np.float64) - m) + a) * s).astype(np.float32)


def _wrapped(a, b):
    """sum_j sum_c a[(k + j + W // 2) mod W, c] b[j, c] for k = 0..W-1 (the correlation's shift structure), fp64; W = a.shape[0]."""
    wd = np.shape(a)[0]
    jj = np.arange(wd)
    idx = (np.arange(wd)[:, None] + jj[None, :] + wd // 2) % wd
    return (np.asarray(a, np.float64) @ np.asarray(b, np.float64).T)[idx, jj[None, :]].sum(axis=1)


def norm_sigma(v, mode):
    """Elementwise error of the stored normalised value against the fp64 truth: one fp32 rounding (u |x'|) plus the fp64 error of the
    statistics carried by s (at most 512 fp64 roundings of |x| in the sums: 2^-44 s max|x|), plus the subnormal floor."""
    if mode == "none":
        return np.zeros(np.shape(v))
    x = np.asarray(v, np.float64)
    _, _, s = affine64(x, mode)
    xn = normalize64(x, mode)
    return E.U32 * np.abs(xn) + 2.0 ** -44 * s * np.abs(x).max(axis=-2, keepdims=True) + E.U_SUB


def corr_norm_pair(l, r, mode):
    """{'corr': fp64 normalised correlation (W,), 'direct' / 'spectral': elementwise bounds ('spectral' at W = 360 only).

    The bound is E.corr_pair's on the fp64-normalised volumes (the correlation kernels' own arithmetic on those operands) plus the
    normalisation's rounding carried through the correlation: with stored values l' + dl, r' + dr the correlation moves by
    sum (l' dr + dl r') + O(d^2); the elementwise errors are independent roundings, so per shift they add in quadrature:
        sigma_k^2 = sum_j sum_c (l'[(k+j+W//2) mod W, c]^2 sigma_r[j, c]^2 + sigma_l[(k+j+W//2) mod W, c]^2 r'[j, c]^2)
    and the bound adds SAFETY sigma_k (SAFETY = 6, as everywhere in oracle/error_bounds.py)."""
    ln, rn = normalize64(l, mode), normalize64(r, mode)
    c = E.corr_pair(ln, rn)
    sl, sr = norm_sigma(l, mode), norm_sigma(r, mode)
    carried = E.SAFETY * np.sqrt(_wrapped(np.square(ln), np.square(sr)) + _wrapped(np.square(sl), np.square(rn)))
    out = {"corr": c["corr"], "direct": c["direct"] + carried}
    if "spectral" in c:
        out["spectral"] = c["spectral"] + carried
    return out


def yaw_ok(gpu_corr_row, gpu_bin, ref_corr, bound):
    """The rule of test_parity_budget for one pair: the GPU's bin is the fp64 first maximum wherever the fp64 top-two gap exceeds
    twice the bound; elsewhere it must be a maximum within the bound (fp64 value at the GPU's bin >= max - 2 bound)."""
    k = int(np.argmax(ref_corr))
    srt = np.sort(ref_corr)
    b = float(np.max(bound))
    if srt[-1] - srt[-2] > 2 * b:
        return int(gpu_bin) == k
    return ref_corr[int(gpu_bin)] >= srt[-1] - 2 * b


def edge_volume(seed=0, width=360):
    """(width, 128) float32: random ReLU channels and dead channels next to the edge channels of every mode -- all zero, constant,
    one non-zero column, negative values, 2^100, 2^-100, subnormals, a small-range channel (the +1e-6 / +1e-5 constants matter)
    and a large near-constant one."""
    rng = np.random.default_rng(seed)
    wd = width
    v = np.maximum(rng.normal(0.2, 1.0, size=(wd, 128)), 0).astype(np.float32)
    v[:, 0:8] = 0                                                            # dead
    v[:, 8] = np.float32(3.25)                                               # constant
    v[:, 9] = 0
    v[int(rng.integers(wd)), 9] = np.float32(2.5)                           # one non-zero column
    v[:, 10] = rng.normal(0.0, 1.0, wd).astype(np.float32)                 # negative values
    v[:, 11] = -np.abs(rng.normal(0.0, 1.0, wd)).astype(np.float32)
    v[:, 12] = (np.float32(2.0 ** 100) * rng.random(wd)).astype(np.float32)
    v[:, 13] = (np.float32(2.0 ** -100) * rng.random(wd)).astype(np.float32)
    v[:, 14] = (rng.random(wd) * 1e-39).astype(np.float32)                 # subnormal
    v[:, 15] = (rng.random(wd) * 3e-7).astype(np.float32)                  # range below the +1e-6 of 'scaling'
    v[:, 16] = (rng.random(wd) * 2e-6).astype(np.float32)                  # values below the +1e-5 of 'standardization'
    v[:, 17] = np.float32(1000.0) + (rng.random(wd) * 0.01).astype(np.float32)   # large, near-constant
    return v


def rolled(v, s):
    """r = l rolled by s columns (r[j] = l[j - s])."""
    return np.roll(np.asarray(v), s, axis=0)


def known_bin(s, W=360):
    """The correlation bin at which r = rolled(l, s) peaks: corr[k] pairs l[(k + j + W // 2) mod W] with r[j] = l[j - s], so the
    peak is where k + W // 2 = -s (mod W)."""
    return (-s - W // 2) % W
