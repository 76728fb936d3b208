"""NumPy statement of the marginal covariances of csrc/pose_graph.hip (ovn_pose_graph_marginals; include/ovn_hip.h, DESIGN.md section
34), in float64 and in the kernels' order of additions.  It builds on tests/_pose_graph_ref.py (R) and tests/_pose_graph_loops_ref.py
(L) and uses their notation.

For the left perturbation T_k <- Exp(eps_k) T_k the diagonal block of H^-1 = H_c^-1 - H_c^-1 J' S^-1 J H_c^-1 at node k is
  Sigma_world(k) = Gamma[k] - Y_k' Y_k,   L_S Y_k = V_k',   V_k = [ (Gamma[clamp(k, lo_a, hi_a)] - Gamma[lo_a]) sigma_a C_a' ]_a
and the two output frames are A Sigma_world A' with A = Ad(T_k^-1) ("local": the optimizer's delta_k) or A = [[I, -p_k^], [0, I]]
("position": position in the world, rotation vector in the world).

Order of additions, as the kernels take them:
  V          M = Gamma[min(k, hi)] - Gamma[lo] entry by entry; V[i][6 a + q] = sigma_a (sum_t M[i][t] C_a[q][t]) in index order; zero for
             k <= lo_a and for an edge that was left out
  sweep      block row by block row of the factor, block 48: x = v - s_0 - s_1 - ... with s_t the 48-term sum over block column t in
             index order, one subtraction per earlier block in block order; inside the diagonal block y_c = x_c / L_cc and one
             subtraction per row below, column by column
  Y'Y        per entry of the lower triangle, the rows of Y in ascending order from 0.0
  Sigma      Gamma[k] - Y'Y on the lower triangle, mirrored; (A Sigma) A' with inner sums in index order; the lower triangle mirrored
`reverse=True` takes every one of these sums backwards, with the reversed forms of R and L underneath; the difference between the two
forms is the rounding noise a test allows the kernel, times ten."""
import numpy as np

from tests import _pose_graph_ref as R
from tests import _pose_graph_loops_ref as L

BLOCK = L.BLOCK
TILE = 8            # PGM_TN: queried nodes per workgroup
CHUNK = 512 * TILE  # PGM_CHUNK * PGM_TN: queried nodes per launch of the sweep
FRAMES = ("local", "position")


def prepare(poses, lin, Omega, reverse=False):
    """What the kernel reads: L.prepare's dictionary for a graph with loop edges; G, N and Gamma alone for a bare chain."""
    if len(lin["edges"]) > lin["n"] - 1:
        return L.prepare(poses, lin, Omega, reverse)
    G, N = R.chain_terms(poses, lin, Omega, reverse)
    return dict(G=G, N=N, gamma=L.gamma(G, reverse), C=np.zeros((0, 6, 6)), span=np.zeros((0, 4)), F=np.zeros((0, 0)), n=lin["n"])


def v_transposed(p, nodes, reverse=False):
    """(sp, 6 K): the columns of V_k' for the queried nodes, the padding rows zero."""
    Gam, C, span = p["gamma"], p["C"], p["span"]
    sp = len(p["F"])
    out = np.zeros((sp, 6 * len(nodes)))
    for a in range(len(C)):
        if not span[a, 3]:
            continue
        lo, hi = int(span[a, 0]), int(span[a, 1])
        for c, k in enumerate(nodes):
            if k > lo:
                M = Gam[min(k, hi)] - Gam[lo]
                out[6 * a:6 * a + 6, 6 * c:6 * c + 6] = (span[a, 2] * R.mm(M, C[a].T.copy(), reverse)).T
    return out


def forward(F, X, block=BLOCK, reverse=False):
    """L_S^-1 X for a matrix of right-hand sides, in the sweep's order."""
    x = np.asarray(X, np.float64).copy()
    sp = len(x)
    for k0 in range(0, sp, block):
        k1 = k0 + block
        for c in range(k0, k1):
            x[c] = x[c] / F[c, c]
            x[c + 1:k1] = x[c + 1:k1] - F[c + 1:k1, c:c + 1] * x[c]
        if k1 < sp:
            x[k1:] = x[k1:] - R.mm(F[k1:, k0:k1], x[k0:k1], reverse)
    return x


def gram(Y, reverse=False):
    """(K,6,6): Y_k' Y_k, the rows in order from 0.0."""
    sp = len(Y)
    Yk = Y.reshape(sp, -1, 6)
    acc = np.zeros((Yk.shape[1], 6, 6))
    for r in (range(sp - 1, -1, -1) if reverse else range(sp)):
        acc = acc + Yk[r][:, :, None] * Yk[r][:, None, :]
    return acc


def mirror(M):
    return np.tril(M) + np.tril(M, -1).T


def position_jacobian(T):
    """d (position, rotation vector in the world) / d eps for T <- Exp(eps) T, eps = (v, omega): [[I, -p^], [0, I]]."""
    J = np.eye(6)
    J[:3, 3:] = -R.hat(T[:3, 3])
    return J


def world(p, nodes, reverse=False):
    """(K,6,6): Sigma_world, symmetric to the bit; nodes inside [0, N)."""
    nodes = [int(k) for k in nodes]
    Gam = p["gamma"]
    if len(p["C"]):
        acc = gram(forward(p["F"], v_transposed(p, nodes, reverse), reverse=reverse), reverse)
        return np.stack([mirror(Gam[k] - acc[c]) for c, k in enumerate(nodes)])
    return np.stack([mirror(Gam[k]) for k in nodes])


def marginals(p, poses, nodes, frame="position", reverse=False):
    """(K,6,6) as ovn_pose_graph_marginals writes them: node 0 all zeros, an id outside [0, N) all NaN."""
    assert frame in FRAMES
    n = p["n"]
    nodes = [int(k) for k in nodes]
    inside = [k for k in nodes if 0 <= k < n]
    Sw = iter(world(p, inside, reverse)) if inside else iter(())
    out = np.zeros((len(nodes), 6, 6))
    for c, k in enumerate(nodes):
        if not 0 <= k < n:
            out[c] = np.nan
            continue
        S = next(Sw)
        if k == 0:
            continue
        A = p["N"][k - 1] if frame == "local" else position_jacobian(poses[k])
        out[c] = mirror(R.mm(R.mm(A, S, reverse), A.T.copy(), reverse))
    return out


def scale(p):
    """The largest entry of Gamma[N - 1]: what the tolerances are relative to."""
    return float(np.abs(p["gamma"][-1]).max())


def distance(a, b, p):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max()) / scale(p)


# ---- the other side: the diagonal blocks of the dense inverse -------------------------------------------------------------------------
def dense_marginals(lin, poses, frame="position"):
    """(N,6,6) from numpy.linalg.inv of the reduced Hessian of the reference linearization (local frame), moved to `frame`."""
    H, free = R.dense_system(lin, 0.0)
    Hi = np.linalg.inv(H)
    out = np.zeros((lin["n"], 6, 6))
    for c, k in enumerate(free):
        S = Hi[6 * c:6 * c + 6, 6 * c:6 * c + 6]
        if frame == "position":
            A = position_jacobian(poses[k]) @ R.adjoint(poses[k])
            S = A @ S @ A.T
        out[k] = S
    return out


# ---- the end-to-end gate: a straight drive that comes back --------------------------------------------------------------------------
GATE = dict(frames=300, step=1.0, out_frames=150, lane=2.0, sigma_t=0.06, sigma_r=0.002, nstd=3.0, min_gap=100)


def gate_drive(g=GATE):
    """300 poses: 150 steps of 1 m along +x, then back along -x on a lane 2 m to the side, heading turned by pi.  Frame 150 + m passes
    frame 149 - m at 2 m.  Exact odometry; Omega from sigma_t, sigma_r."""
    n, half = g["frames"], g["out_frames"]
    poses = np.tile(np.eye(4), (n, 1, 1))
    for k in range(n):
        if k < half:
            poses[k, :3, 3] = [g["step"] * k, 0.0, 0.0]
        else:
            poses[k, :3, :3] = np.diag([-1.0, -1.0, 1.0])
            poses[k, :3, 3] = [g["step"] * (2 * half - 1 - k), g["lane"], 0.0]
    edges = np.array([(k, k + 1) for k in range(n - 1)], np.int32)
    Z = np.stack([R.rel_se3(poses[k], poses[k + 1]) for k in range(n - 1)])
    Om = np.diag([1.0 / g["sigma_t"] ** 2] * 3 + [1.0 / g["sigma_r"] ** 2] * 3)
    fixed = np.zeros(n, bool)
    fixed[0] = True
    return dict(init=poses, edges=edges, Z=Z, Omega=np.stack([Om] * (n - 1)), fixed=fixed, huber=np.inf)


def gate_candidates(g=GATE):
    """frame -> the candidate list lcd.gate_candidates keeps with the restated L = 0 marginals as the search space."""
    from overlapnet_amd import lcd
    d = gate_drive(g)
    lin = R.linearize(d["init"], d["fixed"], d["edges"], d["Z"], d["Omega"], d["huber"])
    cov = marginals(prepare(d["init"], lin, d["Omega"]), d["init"], range(g["frames"]), "position")
    ell = lcd.ellipses_from_covariances(cov, g["nstd"])
    xy = d["init"][:, :2, 3]
    length = lcd.travelled_distances(xy)
    return {k: [int(v) for v in lcd.gate_candidates(k, xy, length, ell[k], inactive_time_thres=g["min_gap"] - 1,
                                                    inactive_dist_thres=-np.inf)] for k in range(g["frames"])}


if __name__ == "__main__":      # python -m tests._pose_graph_marginals_ref > tests/golden/pose_graph_marginals.json
    import json
    cand = gate_candidates()
    print(json.dumps(dict(geometry=GATE, candidates={str(k): v for k, v in cand.items() if v}), indent=1, sort_keys=True))
