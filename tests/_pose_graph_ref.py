"""NumPy statement of the SE(3) pose-graph optimizer of csrc/pose_graph.hip (include/ovn_hip.h), all in float64.

Poses T_i are (4,4) sensor-to-world; an edge (i, j, Z, Omega) measures T_i^-1 T_j; twists are (v, omega), translation first.
  residual   r = Log(Z^-1 T_i^-1 T_j)
  update     T_i <- T_i Exp(delta_i)
  Jacobians  B = dr/d delta_j = J_r^-1(r),  A = dr/d delta_i = -B Ad(T_j^-1 T_i)
  cost       sum rho(s), s = sqrt(r' Omega r), rho = Huber; weight w = 1 or huber / s
  H = sum w J' Omega J,  g = sum w J' Omega r, rows and columns of fixed nodes removed
  outer      Levenberg-Marquardt on (H + lam blockdiag(H)) delta = -g, see `optimize` for the schedule
  inner      preconditioned conjugate gradients, block-Jacobi or odometry-chain preconditioner

Every trigonometric coefficient switches to its series in x = theta^2 below SERIES_X, exactly as the kernel does.  `reverse=True` runs
the same arithmetic with every sum taken in the opposite order (the inner sums of the matrix products, the sums over a node's edges,
the dot products): the difference between the two is the rounding noise a test allows the kernel, times ten."""
import numpy as np

SERIES_X = 1e-2          # theta^2 below which the coefficient series are used (theta < 0.1 rad)
LAMBDA_FIRST = 1e-6      # the damping a rejected Gauss-Newton step starts from
LAMBDA_MAX = 1e8
XTOL = 1e-10             # |delta|_inf at which the outer loop stops


def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def mm(a, b, reverse=False):
    """a @ b with the inner sum in index order (or reversed): products first, then one addition after another."""
    k = a.shape[1]
    out = None
    for t in (range(k - 1, -1, -1) if reverse else range(k)):
        term = a[:, t:t + 1] * b[t:t + 1, :] if b.ndim == 2 else a[:, t] * b[t]
        out = term if out is None else out + term
    return out


def coeffs(x):
    """a = sin t / t, b = (1 - cos t) / t^2, c1 = (t - sin t) / t^3, c2 = (t^2 + 2 cos t - 2) / (2 t^4),
    c3 = (2 t - 3 sin t + t cos t) / (2 t^5), e = 1 / t^2 - (1 + cos t) / (2 t sin t), with x = t^2."""
    if x < SERIES_X:
        a = 1.0 + x * (-1.0 / 6 + x * (1.0 / 120 + x * (-1.0 / 5040 + x * (1.0 / 362880))))
        b = 0.5 + x * (-1.0 / 24 + x * (1.0 / 720 + x * (-1.0 / 40320 + x * (1.0 / 3628800))))
        c1 = 1.0 / 6 + x * (-1.0 / 120 + x * (1.0 / 5040 + x * (-1.0 / 362880 + x * (1.0 / 39916800))))
        c2 = 1.0 / 24 + x * (-1.0 / 720 + x * (1.0 / 40320 + x * (-1.0 / 3628800 + x * (1.0 / 479001600))))
        c3 = 1.0 / 120 + x * (-2.0 / 5040 + x * (3.0 / 362880 + x * (-4.0 / 39916800 + x * (5.0 / 6227020800))))
        e = 1.0 / 12 + x * (1.0 / 720 + x * (1.0 / 30240 + x * (1.0 / 1209600 + x * (1.0 / 47900160))))
        return a, b, c1, c2, c3, e
    t = np.sqrt(x)
    s, c = np.sin(t), np.cos(t)
    return (s / t, (1.0 - c) / x, (t - s) / (x * t), (x + 2.0 * c - 2.0) / (2.0 * x * x),
            (2.0 * t - 3.0 * s + t * c) / (2.0 * x * x * t), 1.0 / x - (1.0 + c) / (2.0 * t * s))


def exp_se3(xi, reverse=False):
    xi = np.asarray(xi, np.float64)
    v, w = xi[:3], xi[3:]
    x = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    a, b, c1, _, _, _ = coeffs(x)
    W = hat(w)
    W2 = mm(W, W, reverse)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + a * W + b * W2
    T[:3, 3] = mm(np.eye(3) + b * W + c1 * W2, v, reverse)
    return T


def log_so3(R):
    ax = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    sn = np.sqrt((ax[0] * ax[0] + ax[1] * ax[1]) + ax[2] * ax[2])
    cs = 0.5 * (((R[0, 0] + R[1, 1]) + R[2, 2]) - 1.0)
    t = np.arctan2(sn, cs)
    x = t * t
    k = 1.0 / coeffs(x)[0] if x < SERIES_X else t / sn
    return k * ax


def log_se3(T, reverse=False):
    w = log_so3(T[:3, :3])
    x = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    e = coeffs(x)[5]
    W = hat(w)
    Vinv = np.eye(3) - 0.5 * W + e * mm(W, W, reverse)
    return np.concatenate([mm(Vinv, T[:3, 3], reverse), w])


def inv_se3(T, reverse=False):
    out = np.eye(4)
    Rt = T[:3, :3].T
    out[:3, :3] = Rt
    out[:3, 3] = -mm(Rt, T[:3, 3], reverse)
    return out


def mul_se3(A, B, reverse=False):
    out = np.eye(4)
    out[:3, :3] = mm(A[:3, :3], B[:3, :3], reverse)
    out[:3, 3] = mm(A[:3, :3], B[:3, 3], reverse) + A[:3, 3]
    return out


def rel_se3(A, B, reverse=False):
    """A^-1 B without forming A^-1's translation first: R = Ra' Rb, t = Ra' (tb - ta)."""
    out = np.eye(4)
    Rt = A[:3, :3].T
    out[:3, :3] = mm(Rt, B[:3, :3], reverse)
    out[:3, 3] = mm(Rt, B[:3, 3] - A[:3, 3], reverse)
    return out


def adjoint(T, reverse=False):
    R, t = T[:3, :3], T[:3, 3]
    Ad = np.zeros((6, 6))
    Ad[:3, :3] = R
    Ad[3:, 3:] = R
    Ad[:3, 3:] = mm(hat(t), R, reverse)
    return Ad


def jl_inv(xi, reverse=False):
    """Inverse left Jacobian of SE(3) at xi = (rho, phi), closed form (Barfoot, State Estimation for Robotics, 7.85-7.86)."""
    rho, phi = xi[:3], xi[3:]
    x = (phi[0] * phi[0] + phi[1] * phi[1]) + phi[2] * phi[2]
    _, _, c1, c2, c3, e = coeffs(x)
    P, F = hat(rho), hat(phi)
    m = lambda a, b: mm(a, b, reverse)
    FP, PF, FF = m(F, P), m(P, F), m(F, F)
    FPF = m(FP, F)
    Q = 0.5 * P + c1 * ((FP + PF) + FPF) + c2 * ((m(F, FP) + m(PF, F)) - 3.0 * FPF) + c3 * (m(FPF, F) + m(F, FPF))
    Ji = np.eye(3) - 0.5 * F + e * FF
    out = np.zeros((6, 6))
    out[:3, :3] = Ji
    out[3:, 3:] = Ji
    out[:3, 3:] = -m(m(Ji, Q), Ji)
    return out


def jr_inv(xi, reverse=False):
    return jl_inv(-np.asarray(xi, np.float64), reverse)


def residual(Ti, Tj, Z, reverse=False):
    return log_se3(rel_se3(Z, rel_se3(Ti, Tj, reverse), reverse), reverse)


def edge_terms(Ti, Tj, Z, reverse=False):
    """r, A = dr/d delta_i, B = dr/d delta_j."""
    Tij = rel_se3(Ti, Tj, reverse)
    r = log_se3(rel_se3(Z, Tij, reverse), reverse)
    B = jr_inv(r, reverse)
    A = -mm(B, adjoint(inv_se3(Tij, reverse), reverse), reverse)
    return r, A, B


def huber(s, k):
    """(rho, weight) of the Huber kernel with threshold k at s >= 0."""
    if s <= k:
        return 0.5 * s * s, 1.0
    return k * (s - 0.5 * k), k / s


def incidence(n, edges):
    """CSR incidence list: node_ptr (n + 1), node_edge (2 E), each node's edges in ascending edge index."""
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    lists = [[] for _ in range(n)]
    for e, (i, j) in enumerate(edges):
        lists[i].append(e)
        lists[j].append(e)
    ptr = np.zeros(n + 1, np.int32)
    ptr[1:] = np.cumsum([len(v) for v in lists])
    flat = np.array([e for v in lists for e in v], np.int32)
    return ptr, flat


def _sum(terms, reverse):
    terms = list(terms)
    if reverse:
        terms = terms[::-1]
    out = terms[0]
    for t in terms[1:]:
        out = out + t
    return out


def tree_sum(v):
    """The kernel's reduction of per-thread values: blocks of 256 by a halving tree, the block sums strided over 256 lanes in order,
    then the same tree."""
    v = np.asarray(v, np.float64)
    def tree(b):
        b = np.concatenate([b, np.zeros(256 - len(b))])
        h = 128
        while h:
            b = b[:h] + b[h:2 * h]
            h //= 2
        return b[0]
    if len(v) == 0:
        return 0.0
    parts = [tree(v[k:k + 256]) for k in range(0, len(v), 256)]
    lanes = np.zeros(256)
    for k, p in enumerate(parts):
        lanes[k % 256] += p
    return tree(lanes)


def linearize(poses, fixed, edges, Z, Omega, k=np.inf, reverse=False, jacobians=True):
    poses, Z, Omega = (np.asarray(a, np.float64) for a in (poses, Z, Omega))
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    n, E = len(poses), len(edges)
    fixed = np.asarray(fixed, bool)
    m = lambda a, b: mm(a, b, reverse)
    out = dict(r=np.zeros((E, 6)), s=np.zeros(E), w=np.zeros(E), A=np.zeros((E, 6, 6)), B=np.zeros((E, 6, 6)), Hii=np.zeros((E, 6, 6)),
               Hij=np.zeros((E, 6, 6)), Hjj=np.zeros((E, 6, 6)), gi=np.zeros((E, 6)), gj=np.zeros((E, 6)), rho=np.zeros(E), bad=0,
               edges=edges, fixed=fixed, n=n)
    for e, (i, j) in enumerate(edges):
        if not (np.isfinite(poses[i]).all() and np.isfinite(poses[j]).all() and np.isfinite(Z[e]).all() and np.isfinite(Omega[e]).all()):
            out["bad"] += 1
            continue
        r, A, B = edge_terms(poses[i], poses[j], Z[e], reverse)
        if not np.isfinite(r).all():
            out["bad"] += 1
            continue
        Or = m(Omega[e], r)
        s = np.sqrt(max(_sum(r * Or, reverse), 0.0))
        rho, w = huber(s, k)
        out["r"][e], out["s"][e], out["w"][e], out["rho"][e] = r, s, w, rho
        if not jacobians:
            continue
        WA, WB = w * m(Omega[e], A), w * m(Omega[e], B)
        out["A"][e], out["B"][e] = A, B
        out["Hii"][e], out["Hij"][e], out["Hjj"][e] = m(A.T, WA), m(A.T, WB), m(B.T, WB)
        out["gi"][e], out["gj"][e] = w * m(A.T, Or), w * m(B.T, Or)
    out["cost"] = tree_sum(out["rho"]) if not reverse else float(_sum(out["rho"], True)) if E else 0.0
    if not jacobians:
        return out
    ptr, flat = incidence(n, edges)
    g, D = np.zeros((n, 6)), np.zeros((n, 6, 6))
    for v in range(n):
        if fixed[v] or ptr[v] == ptr[v + 1]:
            continue
        inc = flat[ptr[v]:ptr[v + 1]]
        g[v] = _sum([out["gi"][e] if edges[e, 0] == v else out["gj"][e] for e in inc], reverse)
        D[v] = _sum([out["Hii"][e] if edges[e, 0] == v else out["Hjj"][e] for e in inc], reverse)
    out["g"], out["D"], out["ptr"], out["flat"] = g, D, ptr, flat
    return out


def matvec(lin, lam, x, reverse=False):
    """(H + lam blockdiag(H)) x per node over its incidence list; fixed rows are 0 and fixed columns are not read."""
    edges, fixed = lin["edges"], lin["fixed"]
    m = lambda a, b: mm(a, b, reverse)
    y = np.zeros_like(x)
    for v in range(lin["n"]):
        if fixed[v]:
            continue
        acc = lam * m(lin["D"][v], x[v])
        for e in (lin["flat"][lin["ptr"][v]:lin["ptr"][v + 1]][::-1] if reverse else lin["flat"][lin["ptr"][v]:lin["ptr"][v + 1]]):
            i, j = edges[e]
            xi = np.zeros(6) if fixed[i] else x[i]
            xj = np.zeros(6) if fixed[j] else x[j]
            if i == v:
                acc = acc + (m(lin["Hii"][e], xi) + m(lin["Hij"][e], xj))
            else:
                acc = acc + (m(lin["Hij"][e].T, xi) + m(lin["Hjj"][e], xj))
        y[v] = acc
    return y


def dense_system(lin, lam):
    """The damped matrix over the FREE nodes and the free index list: (6 F, 6 F), (F,)."""
    n = lin["n"]
    H = np.zeros((6 * n, 6 * n))
    for e, (i, j) in enumerate(lin["edges"]):
        H[6 * i:6 * i + 6, 6 * i:6 * i + 6] += lin["Hii"][e]
        H[6 * j:6 * j + 6, 6 * j:6 * j + 6] += lin["Hjj"][e]
        H[6 * i:6 * i + 6, 6 * j:6 * j + 6] += lin["Hij"][e]
        H[6 * j:6 * j + 6, 6 * i:6 * i + 6] += lin["Hij"][e].T
    for v in range(n):
        H[6 * v:6 * v + 6, 6 * v:6 * v + 6] *= (1.0 + lam)
    free = np.flatnonzero(~lin["fixed"])
    idx = (6 * free[:, None] + np.arange(6)).ravel()
    return H[np.ix_(idx, idx)], free


def dense_solve(lin, lam):
    H, free = dense_system(lin, lam)
    x = np.zeros((lin["n"], 6))
    x[free] = np.linalg.solve(H, -lin["g"][free].ravel()).reshape(-1, 6)
    return x


def chol_inverse(D):
    """Inverse of a 6 x 6 SPD block by Cholesky; None on a non-positive pivot."""
    L = np.zeros((6, 6))
    for c in range(6):
        d = D[c, c]
        for t in range(c):
            d = d - L[c, t] * L[c, t]
        if not d > 0.0:
            return None
        L[c, c] = np.sqrt(d)
        for rr in range(c + 1, 6):
            v = D[rr, c]
            for t in range(c):
                v = v - L[rr, t] * L[c, t]
            L[rr, c] = v / L[c, c]
    Li = np.zeros((6, 6))
    for c in range(6):
        Li[c, c] = 1.0 / L[c, c]
        for rr in range(c + 1, 6):
            v = 0.0
            for t in range(c, rr):
                v = v - L[rr, t] * Li[t, c]
            Li[rr, c] = v / L[rr, rr]
    return mm(Li.T, Li)


def jacobi_blocks(lin):
    out = np.zeros_like(lin["D"])
    for v in range(lin["n"]):
        if not lin["fixed"][v]:
            out[v] = chol_inverse(lin["D"][v])
    return out


def inv3(J):
    """Inverse of a 3 x 3 matrix by cofactors."""
    J = J.ravel()
    c00, c01, c02 = J[4] * J[8] - J[5] * J[7], J[5] * J[6] - J[3] * J[8], J[3] * J[7] - J[4] * J[6]
    d = 1.0 / ((J[0] * c00 + J[1] * c01) + J[2] * c02)
    return np.array([[c00 * d, (J[2] * J[7] - J[1] * J[8]) * d, (J[1] * J[5] - J[2] * J[4]) * d],
                     [c01 * d, (J[0] * J[8] - J[2] * J[6]) * d, (J[2] * J[3] - J[0] * J[5]) * d],
                     [c02 * d, (J[1] * J[6] - J[0] * J[7]) * d, (J[0] * J[4] - J[1] * J[3]) * d]])


def chain_terms(poses, lin, Omega, reverse=False):
    """Per chain edge m (nodes m, m + 1): G_m = P_m (w_m Omega_m)^-1 P_m' with P_m = Ad(T_{m+1}) B_m^-1, and N_m = Ad(T_{m+1}^-1)."""
    n = lin["n"]
    m_ = lambda a, b: mm(a, b, reverse)
    G, N = np.zeros((n - 1, 6, 6)), np.zeros((n - 1, 6, 6))
    for m in range(n - 1):
        B = lin["B"][m]
        Ji = inv3(B[:3, :3])
        Binv = np.zeros((6, 6))
        Binv[:3, :3] = Ji
        Binv[3:, 3:] = Ji
        Binv[:3, 3:] = -m_(m_(Ji, B[:3, 3:]), Ji)
        P = m_(adjoint(poses[m + 1], reverse), Binv)
        Winv = chol_inverse(lin["w"][m] * Omega[m])
        G[m] = m_(m_(P, Winv), P.T)
        N[m] = adjoint(inv_se3(poses[m + 1], reverse), reverse)
    return G, N


def chain_apply(G, N, y):
    """H_chain^-1 y by transforms and cumulative sums; y, result: (n, 6) with row 0 (the fixed node) zero."""
    t = np.einsum("mba,mb->ma", N, y[1:])                       # N' y
    s = np.cumsum(t[::-1], axis=0)[::-1]                        # suffix sums
    u = np.einsum("mab,mb->ma", G, s)
    c = np.cumsum(u, axis=0)                                    # prefix sums
    z = np.zeros_like(y)
    z[1:] = np.einsum("mab,mb->ma", N, c)
    return z


def chain_apply_scan(G, N, y, block=256):
    """chain_apply in the kernel's order of additions: Hillis-Steele inside blocks of `block`, block totals scanned in order."""
    def scan(v):
        n = len(v)
        out = v.copy()
        for b0 in range(0, n, block):
            seg = out[b0:b0 + block].copy()
            d = 1
            while d < block:
                nxt = seg.copy()
                nxt[d:] = seg[d:] + seg[:-d]
                seg = nxt
                d *= 2
            out[b0:b0 + block] = seg
        tot = np.zeros(6)
        for b0 in range(0, n, block):
            last = out[min(b0 + block, n) - 1].copy()
            out[b0:b0 + block] = out[b0:b0 + block] + tot if b0 else out[b0:b0 + block]
            tot = tot + last if b0 else last
        return out
    def bmv(M, v):                                             # M[m] v[m] for every m, the inner sum in index order
        out = M[:, :, 0] * v[:, 0:1]
        for t in range(1, 6):
            out = out + M[:, :, t] * v[:, t:t + 1]
        return out
    t = bmv(np.swapaxes(N, 1, 2), y[1:])
    s = scan(t[::-1])[::-1]
    u = bmv(G, s)
    c = scan(u)
    z = np.zeros_like(y)
    z[1:] = bmv(N, c)
    return z


def pcg(lin, lam, precond, rtol=1e-8, max_iter=1000, reverse=False, dot=None):
    """Preconditioned CG on (H + lam blockdiag H) x = -g from x = 0.  precond(r) -> z.  Stops when sqrt(rz / rz0) <= rtol.
    -> x, iterations, sqrt(rz / rz0)."""
    if dot is None:
        dot = (lambda a, b: float(_sum((a * b).ravel(), True))) if reverse else (lambda a, b: tree_sum(np.sum(a * b, axis=1)))
    x = np.zeros_like(lin["g"])
    r = -lin["g"].copy()
    z = precond(r)
    p = z.copy()
    rz0 = rz = dot(r, z)
    if rz0 == 0.0:
        return x, 0, 0.0
    it, rel = 0, 1.0
    while it < max_iter:
        q = matvec(lin, lam, p, reverse)
        pq = dot(p, q)
        if not pq > 0.0:
            break
        alpha = rz / pq
        x = x + alpha * p
        r = r - alpha * q
        z = precond(r)
        rz_new = dot(r, z)
        beta = rz_new / rz
        rz = rz_new
        it += 1
        rel = np.sqrt(rz / rz0)
        if rel <= rtol:
            break
        p = z + beta * p
    return x, it, rel


def make_precond(kind, poses, lin, Omega, lam, scan=False):
    if kind == "jacobi":
        Di, scale = jacobi_blocks(lin), 1.0 / (1.0 + lam)
        return lambda r: np.stack([scale * mm(Di[v], r[v]) for v in range(lin["n"])])
    G, N = chain_terms(poses, lin, Omega)
    return (lambda r: chain_apply_scan(G, N, r)) if scan else (lambda r: chain_apply(G, N, r))


def retract(poses, delta):
    return np.stack([mul_se3(T, exp_se3(d)) for T, d in zip(poses, delta)])


def optimize(poses, fixed, edges, Z, Omega, k=np.inf, max_iterations=20, preconditioner="jacobi", rtol=1e-8, max_cg=100000,
             solver="pcg"):
    """Levenberg-Marquardt from lam = 0 (a Gauss-Newton start).  Every outer iteration solves (H + lam blockdiag H) delta = -g, forms
    the trial poses T Exp(delta) and accepts them when the cost does not rise.  Accepted: lam <- lam / 10, and 0 once that falls to
    LAMBDA_FIRST or below.  Rejected: lam <- LAMBDA_FIRST from 0, else 10 lam; the loop gives up above LAMBDA_MAX.  It stops, converged,
    after a solve whose |delta|_inf is at most XTOL (that step is still taken if the cost does not rise)."""
    poses = np.asarray(poses, np.float64).copy()
    lin = linearize(poses, fixed, edges, Z, Omega, k)
    cost0 = cost = lin["cost"]
    lam, outer, cg, converged = 0.0, 0, 0, False
    while outer < max_iterations and lam <= LAMBDA_MAX and len(lin["edges"]):
        if solver == "dense":
            delta = dense_solve(lin, lam)
        else:
            delta, it, _ = pcg(lin, lam, make_precond(preconditioner, poses, lin, Omega, lam), rtol, max_cg)
            cg += it
        outer += 1
        trial = retract(poses, delta)
        tcost = linearize(trial, fixed, edges, Z, Omega, k, jacobians=False)["cost"]
        small = float(np.max(np.abs(delta))) <= XTOL
        if tcost <= cost:
            poses, cost = trial, tcost
            lin = linearize(poses, fixed, edges, Z, Omega, k)
            lam = 0.0 if lam / 10.0 <= LAMBDA_FIRST else lam / 10.0
        else:
            lam = LAMBDA_FIRST if lam == 0.0 else 10.0 * lam
        if small:
            converged = True
            break
    return dict(poses=poses, cost_initial=cost0, cost_final=cost, outer_iterations=outer, cg_iterations=cg, converged=converged,
                chi2=lin["s"] ** 2, weights=lin["w"], lin=lin)


# ---- the test graphs -------------------------------------------------------------------------------------------------------------------
def ring(n, loops, seed=0, noise_t=0.02, noise_r=0.004, radius=4.0, sigma_t=0.05, sigma_r=0.01, outlier=None):
    """A loop drive of n poses on a circle (with some roll, pitch and height so that nothing is planar), odometry edges (k, k + 1) and
    `loops` = [(i, j), ...] with noisy measurements; the start is dead reckoning along the odometry.  outlier = (i, j, xi): one more
    edge whose measurement is the true one times Exp(xi).  -> dict true, init, edges, Z, Omega, fixed."""
    rng = np.random.default_rng(seed)
    true = []
    for k in range(n):
        a = 2.0 * np.pi * k / n
        T = exp_se3(np.array([0, 0, 0, 0.05 * np.sin(2 * a), 0.04 * np.cos(3 * a), a + 0.5 * np.pi]))
        T[:3, 3] = [radius * np.cos(a), radius * np.sin(a), 0.3 * np.sin(a)]
        true.append(T)
    true = np.stack(true)
    pairs = [(k, k + 1) for k in range(n - 1)] + list(loops)
    sig = np.array([noise_t] * 3 + [noise_r] * 3)
    Z = [mul_se3(rel_se3(true[i], true[j]), exp_se3(sig * rng.standard_normal(6))) for i, j in pairs]
    if outlier is not None:
        i, j, xi = outlier
        pairs.append((i, j))
        Z.append(mul_se3(rel_se3(true[i], true[j]), exp_se3(np.asarray(xi, np.float64))))
    init = [true[0]]
    for k in range(n - 1):
        init.append(mul_se3(init[-1], Z[k]))
    Om = np.diag([1.0 / sigma_t ** 2] * 3 + [1.0 / sigma_r ** 2] * 3)
    fixed = np.zeros(n, bool)
    fixed[0] = True
    return dict(true=true, init=np.stack(init), edges=np.array(pairs, np.int32), Z=np.stack(Z), Omega=np.stack([Om] * len(pairs)),
                fixed=fixed)


CASES = {
    "n16_loop1": dict(n=16, loops=[(15, 0)], huber=np.inf),
    "n16_outlier": dict(n=16, loops=[(15, 0), (12, 1)], outlier=(4, 11, (3.0, -2.0, 0.5, 0.0, 0.0, 0.7)), huber=1.5),
    "n64_loop2": dict(n=64, loops=[(63, 0), (40, 3)], huber=np.inf),
}


def case(name):
    c = dict(CASES[name])
    k = c.pop("huber")
    g = ring(seed=sorted(CASES).index(name) + 1, **c)
    g["huber"] = k
    return g
