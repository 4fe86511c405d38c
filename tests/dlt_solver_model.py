"""A NumPy model of the DLT null-vector solver (csrc/dlt_solver.hpp) and builders of systems
whose answer is known in closed form.  Test infrastructure: the unmarked guards of
test_dlt_solver_model.py prove on the CPU that each system exercises the path the GPU tests
(test_gpu_dlt_solver.py) claim for it.

The model transcribes the solver literally, in float64, with IEEE `/` and `sqrt` where the
kernels refine the hardware's reciprocal estimates: the Givens fold, the zero-column test,
the 1e-30 pivot guard, the 12 steps of inverse iteration with their 1e-20 stopping rule, the
inertia check of the converged vector, and numpy.linalg.svd where the kernels run their
Jacobi SVD.  It predicts paths and step counts, not bits.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

PATH_ZERO_COLUMN, PATH_INVERSE_ITERATION, PATH_JACOBI = 0, 1, 2


# ------------------------------------------------------------------------------- the model
def givens_fold(R, a):
    a = np.array(a, np.float64)
    for k in range(4):
        if a[k] == 0.0:
            continue
        n2 = R[k, k] * R[k, k] + a[k] * a[k]
        ri = 1.0 / np.sqrt(n2)
        c, s = R[k, k] * ri, a[k] * ri
        R[k, k] = n2 * ri
        a[k] = 0.0
        for l in range(k + 1, 4):
            rk, al = R[k, l], a[l]
            R[k, l] = c * rk + s * al
            a[l] = -s * rk + c * al


def fold(A):
    """Rows of A (2N, 4) folded into the upper-triangular R, in row order."""
    R = np.zeros((4, 4))
    for row in np.asarray(A, np.float64):
        givens_fold(R, row)
    return R


def inverse_iteration(R, threshold=1e-20, max_steps=12, pivot_guard=True):
    """(converged, x, steps run)."""
    with np.errstate(all="ignore"):
        d = np.diag(R)
        dmax = np.abs(d).max()
        if not dmax > 0.0:
            return False, np.full(4, np.nan), 0
        piv = d.copy()
        if pivot_guard:
            small = ~(np.abs(d) > 1e-30 * dmax)
            piv[small] = np.where(d[small] < 0.0, -1e-30, 1e-30) * dmax
        rinv = 1.0 / piv
        x = np.full(4, 0.5)
        for it in range(max_steps):
            z, y = np.zeros(4), np.zeros(4)
            for k in range(4):
                acc = x[k]
                for i in range(k):
                    acc = acc - R[i, k] * z[i]
                z[k] = acc * rinv[k]
            z = z * (1.0 / np.abs(z).max())
            for k in range(3, -1, -1):
                acc = z[k]
                for l in range(k + 1, 4):
                    acc = acc - R[k, l] * y[l]
                y[k] = acc * rinv[k]
            y = y * (1.0 / np.abs(y).max())
            n = 1.0 / np.sqrt(y[0] * y[0] + y[1] * y[1] + y[2] * y[2] + y[3] * y[3])
            y = y * (-n if (y * x).sum() < 0.0 else n)
            dd = ((y - x) ** 2).sum()
            x = y
            if not dd == dd:
                return False, x, it + 1
            if it > 0 and dd < threshold:
                return True, x, it + 1
        return False, x, max_steps


def is_smallest_eigenvector(R, x):
    """Four positive LDL^T pivots of R^T R - mu I, mu = |R x|^2 - 1e-12 tr(R^T R)."""
    with np.errstate(all="ignore"):
        S = R.T @ R
        lam = ((R @ x) ** 2).sum()
        S = S - (lam - 1e-12 * np.trace(S)) * np.eye(4)
        ok = True
        for k in range(4):
            ok = ok and bool(S[k, k] > 0.0)
            if k == 3:
                break
            l = S[k + 1:, k] / S[k, k]
            S[k + 1:, k + 1:] -= np.outer(l, S[k + 1:, k])
        return ok


def solve(A, check=True, **kw):
    """The null vector of A (2N, 4) as the kernels take it: (X (4,), path, steps).  steps is the
    inverse-iteration step count (also on the Jacobi path: the steps run before it gave up, or
    before the inertia check refused what it converged to); check=False is the solver before
    that check existed."""
    R = fold(A)
    zcol = -1
    for k in range(4):
        if not R[:k + 1, k].any():
            zcol = k
    if zcol >= 0:
        return np.eye(4)[zcol], PATH_ZERO_COLUMN, 0
    ok, x, steps = inverse_iteration(R, **kw)
    if ok and (not check or is_smallest_eigenvector(R, x)):
        return x, PATH_INVERSE_ITERATION, steps
    return np.linalg.svd(R)[2][-1], PATH_JACOBI, steps


def point(X):
    with np.errstate(all="ignore"):
        return X[:3] / X[3]


# ------------------------------------------------------------------------------- known answers
H4 = np.array([[1, 1, 1, 1], [1, -1, 1, -1], [1, 1, -1, -1], [1, -1, -1, 1]], np.int64)
H8 = np.kron(H4, np.array([[1, 1], [1, -1]], np.int64))     # Sylvester order of the 8x8 matrix
assert (H8 @ H8.T == 8 * np.eye(8)).all() and (H4 == H4.T).all()


def row_basis(n_views):
    """(2 n_views, 4) integers with orthogonal columns of equal norm."""
    return {2: H4, 4: H8[:, [0, 3, 5, 6]]}[n_views]


def quaternion(a, b, c, d):
    """Left-multiplication matrix of the integer quaternion: orthogonal columns of equal norm."""
    return np.array([[a, -b, -c, -d], [b, a, -d, c], [c, d, a, -b], [d, -c, b, a]], np.int64)


def system(n_views, Q, s):
    """A = M diag(s) Q^T in integers: right singular vectors the columns of Q, singular values
    proportional to s."""
    return row_basis(n_views) @ np.diag(np.asarray(s, np.int64)) @ np.asarray(Q, np.int64).T


def closed_form(Q, s):
    """The point Q[:3, k] / Q[3, k], k = argmin s (the last on a tie), as exact Fractions."""
    s = list(s)
    k = max(i for i in range(4) if s[i] == min(s))
    return [Fraction(int(Q[i][k]), int(Q[3][k])) for i in range(3)]


def is_dyadic(fr):
    return fr.denominator & (fr.denominator - 1) == 0


def affine_cameras(A):
    """Cameras and points that make the f32 design matrix equal the integer A (2N, 4) exactly:
    P[v] = [-A[2v, :3] 0; -A[2v+1, :3] 0; 0 0 0 1], pt[v] = A[2v:2v+2, 3], confidence 1.
    Returns proj (N, 3, 4) and pts (N, 2), float32."""
    A = np.asarray(A)
    n = A.shape[0] // 2
    P = np.zeros((n, 3, 4), np.float32)
    P[:, :2, :3] = -A[:, :3].reshape(n, 2, 3)
    P[:, 2, 3] = 1.0
    return P, A[:, 3].reshape(n, 2).astype(np.float32)


Q1, Q2 = quaternion(1, 2, 3, 4), quaternion(2, 1, -3, 5)

# The spectra, by the path they are built for.
#   jacobi: sigma_3 / sigma_4 <= 2.5 and a start that is not nearly aligned with the null vector:
#           twelve steps cannot converge.  With Q2 the rotations of (16, 8, 3, 2) put the null
#           vector in each of the four columns (kmin); with Q1 two of them leave this class (below).
#   late:   the last steps of inverse iteration or the fallback, whichever the arithmetic reports:
#           sigma ratio 3; ratio 2 or 1.5 with Q1 columns that are 24 and 43 degrees from the start.
#   rank3:  an exactly singular A without a zero column; its smallest pivot folds to rounding
#           level (1e-15 of the largest), not to zero (the 'pivot0' systems below do that).
#   tied:   two equal smallest singular values: any vector of their span.
#   ortho:  the null vector is exactly orthogonal to the start (1/2, 1/2, 1/2, 1/2), which is
#           itself a singular vector (Q = H4) or close to one (Q1, s = (3, 2, 16, 8): column 1 of Q1
#           is (-2, 1, 4, -3)): the iteration settles on the wrong vector and the inertia check
#           sends the point to the Jacobi SVD.
JACOBI = [(16, 8, 3, 2), (2, 16, 8, 3), (16, 8, 5, 4), (10, 10, 10, 9), (16, 8, 10, 4), (16, 8, 2, 5)]
JACOBI_Q2 = [(3, 2, 16, 8), (8, 3, 2, 16)]
LATE = [(16, 8, 3, 1), (16, 8, 12, 4)]
LATE_Q1 = [(1, 2, 4, 8), (8, 3, 2, 16)]
RANK3 = [(8, 4, 2, 0), (0, 8, 4, 2)]
TIED = [(16, 8, 3, 3)]
ORTHO_H = [(8, 4, 2, 1), (2, 1, 4, 8), (8, 4, 1, 2), (7, 5, 3, 2)]
ORTHO_Q1 = [(3, 2, 16, 8)]


def spectral_cases(n_views):
    """[(name, kind, Q, s)] of every system A = M diag(s) Q^T of n_views views."""
    out = []
    for qn, Q, extra in (("q1", Q1, {"late": LATE_Q1, "ortho": ORTHO_Q1}), ("q2", Q2, {"jacobi": JACOBI_Q2}),
                         ("h", H4, {"ortho": ORTHO_H})):
        common = {} if qn == "h" else {"jacobi": JACOBI, "late": LATE, "rank3": RANK3, "tied": TIED}
        for kind in ("jacobi", "late", "rank3", "tied", "ortho"):
            for s in common.get(kind, []) + extra.get(kind, []):
                out.append((f"{kind}-{qn}-{'_'.join(map(str, s))}-n{n_views}", kind, Q, s))
    return out


def pivot0_system(n_views, p, q):
    """An exactly zero pivot without a zero column, on any arithmetic: the first row is
    (p, 0, 0, q) and every later row has zeros in columns 0 and 3, so no rotation ever touches
    R[1..3][3] and R = [[|p|, 0, 0, +-q], ..., [0, 0, 0, 0]].  Rank 3, null vector (q, 0, 0, -p)."""
    rows = [(p, 0, 0, q), (0, 2, 1, 0), (0, 1, 3, 0), (0, 1, -1, 0), (0, 3, 1, 0), (0, -1, 2, 0), (0, 2, 2, 0), (0, 1, 0, 0)]
    return np.array(rows[:2 * n_views], np.int64), [Fraction(-q, p), Fraction(0), Fraction(0)]


def cases(n_views):
    """[(name, kind, A (2N, 4) int64, closed-form point [Fraction] * 3)] of every exact system."""
    out = [(name, kind, system(n_views, Q, s), closed_form(Q, s)) for name, kind, Q, s in spectral_cases(n_views)]
    for p, q in ((2, 1), (-4, 3)):       # kind 'pivot0': the 1e-30 pivot guard of inverse iteration
        out.append((f"pivot0-{p}_{q}-n{n_views}", "pivot0") + pivot0_system(n_views, p, q))
    return out


def batch(n_views, kinds=None):
    """The exact systems of n_views views as one DLT batch: the cameras belong to the batch entry,
    so each system is a batch entry of its own with one joint.  Returns (names, kinds,
    proj (B, N, 3, 4), pts (B, N, 1, 2), A (B, 2N, 4) int64, expected [[Fraction] * 3] * B)."""
    cs = [c for c in cases(n_views) if kinds is None or c[1] in kinds]
    A = np.stack([c[2] for c in cs])
    cams = [affine_cameras(a) for a in A]
    proj = np.stack([c[0] for c in cams])
    pts = np.stack([c[1] for c in cams])[:, :, None, :]
    return [c[0] for c in cs], [c[1] for c in cs], proj, pts, A, [c[3] for c in cs]


# ------------------------------------------------------------------------------- physical cameras
def near_coincident(seed, baseline=0.05, depth=3000.0, focal=1000.0, noise=5.0):
    """Two pinhole views a baseline (mm) apart looking down z at a point `depth` away, pixels
    with Gaussian noise: proj (2, 3, 4), pts (2, 2) float32.  The two smallest singular values
    of the system are close: the depth is all but unobservable."""
    rng = np.random.default_rng(seed)
    X = np.array([rng.uniform(-500, 500), rng.uniform(-500, 500), depth, 1.0])
    P = np.zeros((2, 3, 4))
    for v in range(2):
        P[v, :, :3] = np.diag([focal, focal, 1.0])
        P[v, 0, 3] = -focal * baseline * v
    h = P @ X
    pts = h[:, :2] / h[:, 2:3] + noise * rng.standard_normal((2, 2))
    return P.astype(np.float32), pts.astype(np.float32)


def sigma_ratio(A):
    s = np.linalg.svd(np.asarray(A, np.float64), compute_uv=False)
    return s[2] / s[3]


# ------------------------------------------------------------------------------- backward
def backward_closed_form(P, pts, conf, gp):
    """The closed form of mvn_dlt_backward (csrc/backward.hip's header comment) in float64 from
    numpy's eigendecomposition, for one point: P (N, 3, 4), pts (N, 2), conf (N,), gp (3,) ->
    (grad_pts (N, 2), grad_conf (N,))."""
    P, pts, conf, gp = (np.asarray(a, np.float64) for a in (P, pts, conf, gp))
    n = P.shape[0]
    rows = pts.reshape(n, 2, 1) * P[:, 2:3, :] - P[:, :2, :]          # pt P_2 - P_r
    A = (conf.reshape(n, 1, 1) * rows).reshape(-1, 4)
    lam, V = np.linalg.eigh(A.T @ A)                                  # ascending: column 0 is the null vector
    X = V[:, 0]
    gX = np.append(gp / X[3], -(gp @ X[:3]) / X[3] ** 2)
    G = sum(((gX @ V[:, k]) / (lam[0] - lam[k])) * np.outer(V[:, k], X) for k in range(1, 4))
    gA = (A @ (G + G.T)).reshape(n, 2, 4)
    return conf.reshape(n, 1) * (gA * P[:, 2:3, :]).sum(-1), (gA * rows).sum((-1, -2))


# seeds of near_coincident used on the GPU: sigma_3 / sigma_4 = 5.8 (8 steps in the model), 3.0
# (12 steps), 7.6 (7 steps), and the three of the first 400 seeds with a ratio below 2.6 (Jacobi)
NEAR_SEEDS = (1, 2, 6, 14, 113, 176)
NEAR_JACOBI_SEEDS = (14, 113, 176)


def near_coincident_batch(seeds=NEAR_SEEDS):
    """proj (B, 2, 3, 4), pts (B, 2, 1, 2): one batch entry per seed."""
    cams = [near_coincident(s) for s in seeds]
    return np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams])[:, :, None, :]


# exact systems whose gradient is defined (a simple smallest singular value) and whose float64
# reference is too: torch's SVD backward divides by the difference of every pair of singular
# values, so (10, 10, 10, 9) is NaN there although the null vector's gradient exists.  With the
# fixed upstream gradients and per-view confidences of the backward test.
def backward_names(n_views):
    return [name for name, kind, _, s in spectral_cases(n_views)
            if kind in ("jacobi", "late", "ortho") and len(set(s)) == 4]


BACKWARD_GOUT = np.array([[1, -2, 3], [-3, 1, 2], [2, 3, -1]], np.float32)


def backward_conf(n_views):
    return np.array([1, 2, 4, 2][:n_views], np.float32)
