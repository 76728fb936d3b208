"""NumPy statement of the chain-plus-loops inverse of csrc/pose_graph.hip (ovn_pose_graph_loops_*; include/ovn_hip.h, DESIGN.md
section 33), in float64 and in the kernels' order of additions.  It builds on tests/_pose_graph_ref.py (R) and uses its notation.

The graph is a chain (edges 0 .. N-2 = (m, m+1), node 0 fixed) plus L loop edges a = (i, j).  With x = J_c^-1 y,
  J_a x = sigma_a C_a sum_{m in [lo_a, hi_a)} P_m y_m,   C_a = B_a Ad(T_j^-1), lo = min(i, j), hi = max(i, j), sigma = +1 for j > i else -1
  S_ab  = delta_ab (w_a Omega_a)^-1 + sigma_a sigma_b C_a (Gamma[min hi] - Gamma[max lo]) C_b'   where the spans overlap
  Gamma[k] = sum_{m<k} G_m
  H^-1 r: s = suffix(N' r), c = prefix(G s), v_a = sigma_a C_a (c[hi_a - 1] - c[lo_a - 1]), d = S^-1 v,
          e = prefix(sum_{lo_a = m} sigma_a C_a' d_a - sum_{hi_a = m} sigma_a C_a' d_a), z = N prefix(G (s - e))

Order of additions, as the kernels take them:
  scans      Hillis-Steele inside blocks of 256, the block totals added in block order (`scan`)
  6 x 6      every inner sum in index order (R.mm)
  S          M = Gamma[hi] - Gamma[lo]; (C_a M) C_b'; times sigma_a sigma_b; a diagonal block takes its lower triangle for both and
             then (w Omega)^-1 + block
  Cholesky   blocked, right-looking, block 48: in the diagonal block and in the rows below it L_rc = (A_rc - L_r0 L_c0 - L_r1 L_c1 ...)
             / L_cc, one subtraction per earlier column of the block in column order; the trailing matrix takes A_rc - (sum_t L_rt L_ct)
             with the 48-term sum in index order and ONE subtraction
  S^-1 v     block column by block column; inside the diagonal block one subtraction per column (forward ascending, backward
             descending), every other entry one subtraction of a 48-term sum in index order
  e          a chain edge's terms over its node's incidence list in list order
`reverse=True` takes every one of these sums backwards (the prefix sums from the element down, the inner sums from the last index,
the incidence lists from their end); the difference between the two forms is the rounding noise a test allows the kernel, times ten."""
import numpy as np

from tests import _pose_graph_ref as R

BLOCK = 48          # PGL_NB
MAX_LOOPS = 256     # OVN_POSE_GRAPH_MAX_LOOPS


# ---- sums -----------------------------------------------------------------------------------------------------------------------------
def scan(v, block=256, reverse=False):
    """Inclusive prefix sums of the rows of v (n, w) in the kernel's order; reverse: row k is v[k] + v[k-1] + ... + v[0]."""
    v = np.asarray(v, np.float64)
    n = len(v)
    if reverse:
        out = v.copy()
        for t in range(1, n):
            out[t:] = out[t:] + v[:n - t]
        return out
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
    tot = np.zeros(v.shape[1:])
    for b0 in range(0, n, block):
        last = out[min(b0 + block, n) - 1].copy()
        if b0:
            out[b0:b0 + block] = out[b0:b0 + block] + tot
        tot = tot + last if b0 else last
    return out


def bmv(M, v, reverse=False):
    """M[m] v[m] for every m, the inner sum in index order."""
    order = range(5, -1, -1) if reverse else range(6)
    out = None
    for t in order:
        term = M[:, :, t] * v[:, t:t + 1]
        out = term if out is None else out + term
    return out


def gamma(G, reverse=False):
    """(n + 1, 6, 6): Gamma[k] = sum_{m<k} G_m."""
    n = len(G)
    out = np.zeros((n + 1, 6, 6))
    out[1:] = scan(G.reshape(n, 36), reverse=reverse).reshape(n, 6, 6)
    return out


# ---- per loop edge --------------------------------------------------------------------------------------------------------------------
def loop_terms(poses, lin, Omega, reverse=False):
    """C (L,6,6), Winv (L,6,6), span (L,4: lo, hi, sigma, live), left_out, failed -- of the edges after the chain."""
    n = lin["n"]
    edges = lin["edges"][n - 1:]
    L = len(edges)
    C, Winv, span = np.zeros((L, 6, 6)), np.tile(np.eye(6), (L, 1, 1)), np.zeros((L, 4))
    left_out = failed = 0
    for a, (i, j) in enumerate(edges):
        e = n - 1 + a
        if not lin["w"][e] > 0.0:
            left_out += 1
            continue
        Wi = R.chol_inverse(lin["w"][e] * Omega[e])
        if Wi is None or not np.isfinite(Wi).all():
            failed += 1
            continue
        Winv[a] = Wi
        C[a] = R.mm(lin["B"][e], R.adjoint(R.inv_se3(poses[j], reverse), reverse), reverse)
        span[a] = (min(i, j), max(i, j), 1.0 if j > i else -1.0, 1.0)
    return C, Winv, span, left_out, failed


def assemble(Gam, C, Winv, span, reverse=False, block=BLOCK):
    """S padded to a multiple of `block` with an identity diagonal: (sp, sp)."""
    L = len(C)
    sp = (6 * L + block - 1) // block * block
    S = np.eye(sp)
    for a in range(L):
        for b in range(a, L):
            out = np.zeros((6, 6))
            if span[a, 3] and span[b, 3]:
                lo, hi = int(max(span[a, 0], span[b, 0])), int(min(span[a, 1], span[b, 1]))
                if lo < hi:
                    M = Gam[hi] - Gam[lo]
                    out = (span[a, 2] * span[b, 2]) * R.mm(R.mm(C[a], M, reverse), C[b].T, reverse)
            if a == b:
                out = np.tril(out) + np.tril(out, -1).T
                out = Winv[a] + out
            S[6 * a:6 * a + 6, 6 * b:6 * b + 6] = out
            S[6 * b:6 * b + 6, 6 * a:6 * a + 6] = out.T
    return S


# ---- the dense factorization and its solves -------------------------------------------------------------------------------------------
def cholesky_blocked(S, block=BLOCK, reverse=False):
    """-> the lower factor (zero above the diagonal) and the number of pivots that were not positive and finite (replaced by 1)."""
    A = np.tril(np.asarray(S, np.float64))
    sp = len(A)
    fails = 0
    for k0 in range(0, sp, block):
        k1 = k0 + block
        for c in range(k0, k1):
            ts = range(c - 1, k0 - 1, -1) if reverse else range(k0, c)
            d = A[c, c]
            for t in ts:
                d = d - A[c, t] * A[c, t]
            ok = d > 0.0 and np.isfinite(d)
            fails += 0 if ok else 1
            l = np.sqrt(d if ok else 1.0)
            v = A[c + 1:, c].copy()
            for t in ts:
                v = v - A[c + 1:, t] * A[c, t]
            A[c + 1:, c] = v / l
            A[c, c] = l
        if k1 < sp:
            P = A[k1:, k0:k1]
            A[k1:, k1:] = np.tril(A[k1:, k1:] - R.mm(P, P.T.copy(), reverse))
    return A, fails


def solve_factor(F, v, block=BLOCK, reverse=False):
    """S^-1 v from the factor: L y = v, then L' d = y."""
    x = np.asarray(v, np.float64).copy()
    sp = len(x)
    for k0 in range(0, sp, block):
        k1 = k0 + block
        for c in range(k0, k1):
            x[c] = x[c] / F[c, c]
            x[c + 1:k1] = x[c + 1:k1] - F[c + 1:k1, c] * x[c]
        if k1 < sp:
            x[k1:] = x[k1:] - R.mm(F[k1:, k0:k1], x[k0:k1], reverse)
    for k0 in range(sp - block, -1, -block):
        k1 = k0 + block
        for c in range(k1 - 1, k0 - 1, -1):
            x[c] = x[c] / F[c, c]
            x[k0:c] = x[k0:c] - F[c, k0:c] * x[c]
        if k0 > 0:
            x[:k0] = x[:k0] - R.mm(F[k0:k1, :k0].T.copy(), x[k0:k1], reverse)
    return x


# ---- the apply ------------------------------------------------------------------------------------------------------------------------
def prepare(poses, lin, Omega, reverse=False):
    """Everything ovn_pose_graph_loops_prepare writes: G, N, Gamma, C, Winv, span, S, F, pivots, left_out."""
    G, N = R.chain_terms(poses, lin, Omega, reverse)
    Gam = gamma(G, reverse)
    C, Winv, span, left_out, failed = loop_terms(poses, lin, Omega, reverse)
    S = assemble(Gam, C, Winv, span, reverse)
    F, fails = cholesky_blocked(S, reverse=reverse)
    return dict(G=G, N=N, gamma=Gam, C=C, Winv=Winv, span=span, S=S, F=F, pivots=fails + failed, left_out=left_out, n=lin["n"],
                ptr=lin["ptr"], flat=lin["flat"])


def apply(p, y, reverse=False):
    """H^-1 y (undamped); y, result: (n, 6) with row 0 (the fixed node) zero."""
    G, N, C, span, n = p["G"], p["N"], p["C"], p["span"], p["n"]
    L = len(C)
    t = bmv(np.swapaxes(N, 1, 2), y[1:], reverse)
    s = scan(t[::-1], reverse=reverse)[::-1]
    c = scan(bmv(G, s, reverse), reverse=reverse)
    v = np.zeros(len(p["F"]))
    for a in range(L):
        if span[a, 3]:
            lo, hi = int(span[a, 0]), int(span[a, 1])
            diff = c[hi - 1] - (c[lo - 1] if lo > 0 else 0.0)
            v[6 * a:6 * a + 6] = span[a, 2] * R.mm(C[a], diff, reverse)
    d = solve_factor(p["F"], v, reverse=reverse)
    D = np.zeros((n - 1, 6))
    for m in range(n - 1):
        inc = p["flat"][p["ptr"][m]:p["ptr"][m + 1]]
        for e in (inc[::-1] if reverse else inc):
            a = e - (n - 1)
            if a < 0 or not span[a, 3]:
                continue
            t6 = span[a, 2] * R.mm(C[a].T, d[6 * a:6 * a + 6], reverse)
            if int(span[a, 0]) == m:
                D[m] = D[m] + t6
            elif int(span[a, 1]) == m:
                D[m] = D[m] - t6
    e_ = scan(D, reverse=reverse)
    c2 = scan(bmv(G, s - e_, reverse), reverse=reverse)
    z = np.zeros_like(y)
    z[1:] = bmv(N, c2, reverse)
    return z


def make_precond(poses, lin, Omega, reverse=False):
    p = prepare(poses, lin, Omega, reverse)
    return lambda r: apply(p, r, reverse)


def restrict(lin, n_edges):
    """The linearization of the graph with only the first n_edges edges (the per-edge terms are shared, the node sums are redone)."""
    keys = ("r", "s", "w", "A", "B", "Hii", "Hij", "Hjj", "gi", "gj", "rho", "edges")
    out = {k: lin[k][:n_edges] for k in keys}
    out.update(fixed=lin["fixed"], n=lin["n"], bad=lin["bad"], cost=R.tree_sum(out["rho"]))
    n, edges = lin["n"], out["edges"]
    ptr, flat = R.incidence(n, edges)
    g, D = np.zeros((n, 6)), np.zeros((n, 6, 6))
    for v in range(n):
        if lin["fixed"][v] or ptr[v] == ptr[v + 1]:
            continue
        inc = flat[ptr[v]:ptr[v + 1]]
        g[v] = R._sum([out["gi"][e] if edges[e, 0] == v else out["gj"][e] for e in inc], False)
        D[v] = R._sum([out["Hii"][e] if edges[e, 0] == v else out["Hjj"][e] for e in inc], False)
    out.update(g=g, D=D, ptr=ptr, flat=flat)
    return out


# ---- the closed form's other side: S as J H_chain^-1 J', column by column ------------------------------------------------------------
def capacitance_by_columns(poses, lin, Omega):
    n = lin["n"]
    G, N = R.chain_terms(poses, lin, Omega)
    loops = lin["edges"][n - 1:]
    L = len(loops)
    S = np.zeros((6 * L, 6 * L))
    for a, (i, j) in enumerate(loops):
        for q in range(6):
            y = np.zeros((n, 6))
            y[i] += lin["A"][n - 1 + a][q]
            y[j] += lin["B"][n - 1 + a][q]
            y[0] = 0.0
            z = R.chain_apply(G, N, y)
            for b, (k, l) in enumerate(loops):
                S[6 * b:6 * b + 6, 6 * a + q] = lin["A"][n - 1 + b] @ z[k] + lin["B"][n - 1 + b] @ z[l]
        S[6 * a:6 * a + 6, 6 * a:6 * a + 6] += np.linalg.inv(lin["w"][n - 1 + a] * Omega[n - 1 + a])
    return S


# ---- the test graphs ------------------------------------------------------------------------------------------------------------------
MIXED_LOOPS = [(9, 4), (0, 7), (5, 15), (2, 12), (4, 9), (1, 3), (10, 13), (5, 15)]


def mixed():
    """16 poses; loop edges with i > j, touching node 0, ending at node N - 1, nested ((2, 12) around (4, 9)), disjoint ((1, 3) and
    (10, 13)) and identical spans ((9, 4) and (4, 9); (5, 15) twice)."""
    g = R.ring(16, MIXED_LOOPS, seed=11)
    g["huber"] = np.inf
    return g


TWO_LAP_N = 600
TWO_LAP_LOOPS = (7, 8, 9, 17)        # 6 L = 42, 48, 54, 102: one 6-block under, on and over the block size 48, and 2 * 48 + 6
_TWO_LAP_KS = [255, 256, 257, 0, 299, 100, 200, 50, 150, 250, 30, 130, 230, 70, 170, 270, 10]


def two_lap(loops=max(TWO_LAP_LOOPS), n=TWO_LAP_N, seed=21, noise_t=0.02, noise_r=0.004, sigma_t=0.05, sigma_r=0.01):
    """Two laps of a circle of n poses with 0.5 m steps; loop edge a = (k_a + n / 2, k_a) joins the second lap to the first.  The first
    k are 255, 256, 257 -- span ends on both sides of the scans' block boundary at 256 -- and every span [k, k + 300) crosses 256
    or 512.  The first L loop edges of the largest graph are the graph of L loop edges: `restrict` gives its linearization."""
    rng = np.random.default_rng(seed)
    ang = 4.0 * np.pi * np.arange(n) / n
    radius = 0.5 * n / (4.0 * np.pi)
    true = []
    for k in range(n):
        T = R.exp_se3(np.array([0, 0, 0, 0.05 * np.sin(2 * ang[k]), 0.04 * np.cos(3 * ang[k]), ang[k] + 0.5 * np.pi]))
        T[:3, 3] = [radius * np.cos(ang[k]), radius * np.sin(ang[k]), 0.3 * np.sin(ang[k])]
        true.append(T)
    true = np.stack(true)
    pairs = [(k, k + 1) for k in range(n - 1)] + [(k + n // 2, k) for k in _TWO_LAP_KS[:loops]]
    sig = np.array([noise_t] * 3 + [noise_r] * 3)
    Z = [R.mul_se3(R.rel_se3(true[i], true[j]), R.exp_se3(sig * rng.standard_normal(6))) for i, j in pairs]
    init = [true[0]]
    for k in range(n - 1):
        init.append(R.mul_se3(init[-1], Z[k]))
    Om = np.diag([1.0 / sigma_t ** 2] * 3 + [1.0 / sigma_r ** 2] * 3)
    fixed = np.zeros(n, bool)
    fixed[0] = True
    return dict(true=true, init=np.stack(init), edges=np.array(pairs, np.int32), Z=np.stack(Z), Omega=np.stack([Om] * len(pairs)),
                fixed=fixed, huber=np.inf)


def cut(g, loops):
    """The two-lap graph with its first `loops` loop edges."""
    e = len(g["init"]) - 1 + loops
    out = dict(g)
    out.update(edges=g["edges"][:e], Z=g["Z"][:e], Omega=g["Omega"][:e])
    return out


def graphs():
    """name -> graph, the graphs of tests/test_gpu_pose_graph_loops.py and of tests/golden/pose_graph_loops.json."""
    out = {name: R.case(name) for name in sorted(R.CASES)}
    out["mixed"] = mixed()
    big = two_lap()
    for L in TWO_LAP_LOOPS:
        out["two_lap_L%d" % L] = cut(big, L)
    return out


LAMBDAS = {"lam0": 0.0, "lam1e-6": 1e-6}


def golden_entry(g, lin=None):
    """Per lambda: the restated PCG's iterations to rtol 1e-8 and |delta - dense|_inf."""
    if lin is None:
        lin = R.linearize(g["init"], g["fixed"], g["edges"], g["Z"], g["Omega"], g["huber"])
    pre = make_precond(g["init"], lin, g["Omega"])
    out = {}
    for key, lam in LAMBDAS.items():
        x, it, rel = R.pcg(lin, lam, pre, 1e-8, 200)
        out[key] = dict(iterations=int(it), relative_residual=float(rel),
                        dense_distance=float(np.abs(x - R.dense_solve(lin, lam)).max()))
    return out


if __name__ == "__main__":      # python -m tests._pose_graph_loops_ref > tests/golden/pose_graph_loops.json
    import json
    gs = graphs()
    big = two_lap()
    big_lin = R.linearize(big["init"], big["fixed"], big["edges"], big["Z"], big["Omega"], big["huber"])
    table = {}
    for name, g in gs.items():
        lin = restrict(big_lin, len(g["edges"])) if name.startswith("two_lap") else None
        table[name] = golden_entry(g, lin)
    print(json.dumps(table, indent=1, sort_keys=True))
