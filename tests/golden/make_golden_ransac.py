"""Capture the RANSAC triangulation fixture from the REFERENCE implementation.

Run in the build container only (it needs /root/reference and scipy; the GPU box never runs it):

    python -B tests/golden/make_golden_ransac.py

The reference (learnable-triangulation-pytorch, mvn/models/triangulation.py:72-128 and
mvn/utils/multiview.py:104-129, 177-184) is imported read-only with ``cv2`` and ``easydict``
replaced by empty in-memory modules.  ``RANSACTriangulationNet.triangulate_ransac``
is called unbound (it never touches ``self``), with ``random.sample`` bound, for the duration of
the call, to a function that hands out a pair list drawn here, so the fixture records exactly the
hypotheses the reference evaluated.

Inputs come from ``mvn_rocm.synth.algebraic_batch`` (2 px noise); chosen views are displaced by
80-250 px in a random direction.  The reference sees the float32 inputs widened to float64 (its
own callers hand it integer keypoints, which numpy promotes to float64 the same way).

Only data is written, to ``ransac.npz`` next to this script: per case the inputs, the pair lists,
the reference's point and inlier set with ``direct_optimization`` off and on, its reprojection-error
matrix, and for the refined point
  * ``xstar``: a polished minimiser of the reference's cost 1/2 sum rho(r_v^2) -- the reference's
    own least_squares call with ftol = xtol = gtol = 1e-15, continued with float64 damped Newton
    steps until a further step moves the point by less than 1e-6 mm; the lowest-cost point seen;
  * ``ref_cost``: the reference's cost at its own (default-tolerance) answer;
  * ``cost_slack``: the largest cost change among the float32 neighbours of ``xstar`` -- what
    rounding a point to float32 can cost.
The script asserts that xstar costs no more than either reference answer, that no hypothesis's
reprojection error lies within 1e-3 of epsilon (inlier sets are decidable), and that no
hypothesis's two smallest singular values are close (its null vector is well defined).  It prints
|x_ref - xstar| per case: the reference's own distance from the minimum.
"""
from __future__ import annotations

import itertools
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
REF = "/root/reference"
sys.path.insert(0, os.path.join(REPO, "learnable-triangulation-pytorch_amd"))

from mvn_rocm import synth  # noqa: E402  (pure numpy/torch; no GPU needed)

EPSILON = 15.0

# name, B, N, J, outlier views per point, pairs: ('point', n) | ('shared', n) | ('all',)
CASES = [
    ("n4_out1", 2, 4, 17, 1, ("point", 10)),
    ("n5_out2", 2, 5, 17, 2, ("point", 10)),
    ("n2_pair", 2, 2, 17, 0, ("shared", 1)),
    ("n8_out3_all", 1, 8, 17, 3, ("all",)),
    ("n4_clean_one", 2, 4, 17, 0, ("point", 1)),
    ("n4_shared", 3, 4, 5, 1, ("shared", 6)),
    ("n4_j1", 3, 4, 1, 1, ("point", 10)),
]


def import_reference():
    sys.dont_write_bytecode = True
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    easydict = types.ModuleType("easydict")
    easydict.EasyDict = dict
    sys.modules.setdefault("easydict", easydict)
    sys.path.insert(0, REF)
    from mvn.models.triangulation import RANSACTriangulationNet  # noqa: WPS433
    from mvn.utils import multiview  # noqa: WPS433
    return RANSACTriangulationNet, multiview


def reference_ransac(net, proj, pts, pairs, direct):
    """The reference on one point, consuming exactly `pairs` through random.sample."""
    it = iter(pairs)
    orig = random.sample
    random.sample = lambda population, k: [int(v) for v in next(it)]
    try:
        x, inl = net.triangulate_ransac(None, proj, pts, n_iters=len(pairs),
                                        reprojection_error_epsilon=EPSILON, direct_optimization=direct)
    finally:
        random.sample = orig
    assert next(it, None) is None
    return np.asarray(x, np.float64), np.asarray(inl)


def residuals(x, proj, pts):
    """e_v = (pt_v - proj_v(x)) / 2, (n, 2), float64 -- multiview.py:180-181 before the norm."""
    h = proj[:, :, :3] @ x + proj[:, :, 3]
    return 0.5 * (pts - h[:, :2] / h[:, 2:])


def cost(x, proj, pts):
    z = (residuals(x, proj, pts) ** 2).sum(1)
    return 0.5 * np.where(z <= 1.0, z, 2.0 * np.sqrt(z) - 1.0).sum()


def polish(x, proj, pts, max_trials=2000):
    """Damped Newton on `cost` (Gauss-Newton in the residuals, exact in the Huber tail) until an
    accepted step moves the point by less than 1e-6 (mm)."""
    def lin(x):
        h = proj[:, :, :3] @ x + proj[:, :, 3]
        u = h[:, :2] / h[:, 2:]
        e = 0.5 * (pts - u)
        Jm = -0.5 * (proj[:, :2, :3] - u[:, :, None] * proj[:, 2:3, :3]) / h[:, 2, None, None]   # (n, 2, 3)
        z = (e ** 2).sum(1)
        q = np.einsum("nck,nc->nk", Jm, e)
        tail = z > 1.0
        w1 = np.where(tail, 1.0 / np.sqrt(np.maximum(z, 1e-300)), 1.0)
        w2 = np.where(tail, w1 / np.maximum(z, 1e-300), 0.0)
        g = (w1[:, None] * q).sum(0)
        H = np.einsum("n,nca,ncb->ab", w1, Jm, Jm) - np.einsum("n,na,nb->ab", w2, q, q)
        return g, H
    c = cost(x, proj, pts)
    lam = 1e-3
    g, H = lin(x)
    for _ in range(max_trials):
        if not g.any():
            break
        d = -np.linalg.solve(H + lam * np.diag(np.diag(H)) + 1e-300 * np.eye(3), g)
        ct = cost(x + d, proj, pts)
        if ct <= c:
            x, c = x + d, ct
            g, H = lin(x)
            lam = max(lam * 0.1, 1e-12)
            if np.linalg.norm(d) < 1e-6:
                break
        else:
            lam *= 10.0
            if lam > 1e12:
                break
    return x


def f32_neighbour_slack(x, proj, pts):
    xf = x.astype(np.float32)
    lo, hi = np.nextafter(xf, np.float32(-np.inf)), np.nextafter(xf, np.float32(np.inf))
    c0 = cost(x, proj, pts)
    worst = 0.0
    for pick in itertools.product(range(3), repeat=3):
        nb = np.array([(lo, xf, hi)[p][i] for i, p in enumerate(pick)], np.float64)
        worst = max(worst, abs(cost(nb, proj, pts) - c0))
    return worst


def draw_pairs(rng, n_views, n, must_hit=None):
    """n sorted pairs of distinct views; with must_hit every pair contains one of those views."""
    out = []
    while len(out) < n:
        a, b = sorted(rng.choice(n_views, size=2, replace=False).tolist())
        if must_hit is None or a in must_hit or b in must_hit:
            out.append((a, b))
    return out


def capture(net, multiview, name, B, N, J, n_out, pairs_spec, seed):
    from scipy.optimize import least_squares
    rng = np.random.default_rng(seed)
    ab = synth.algebraic_batch(B, N, J, seed=seed)
    proj32 = ab.proj.numpy().copy()
    pts = ab.points.numpy().astype(np.float64)
    outlier = np.zeros((B, J, N), bool)
    for b in range(B):
        for j in range(J):
            for v in rng.choice(N, size=n_out, replace=False):
                ang, mag = rng.uniform(0, 2 * np.pi), rng.uniform(80.0, 250.0)
                pts[b, v, j] += mag * np.array([np.cos(ang), np.sin(ang)])
                outlier[b, j, v] = True
    pts32 = pts.astype(np.float32)
    proj, pts = proj32.astype(np.float64), pts32.astype(np.float64)

    if pairs_spec[0] == "all":
        pairs = np.array(list(itertools.combinations(range(N), 2)), np.int32)
    elif pairs_spec[0] == "shared":
        pairs = np.array(sorted(set(itertools.combinations(range(N), 2)))[:pairs_spec[1]] if N == 2
                         else draw_pairs(rng, N, pairs_spec[1]), np.int32)
    else:
        pairs = np.zeros((B, J, pairs_spec[1], 2), np.int32)
        for b in range(B):
            for j in range(J):
                # the first point of the two-outlier case never draws a clean pair: its best
                # hypothesis has exactly two inliers
                hit = set(np.nonzero(outlier[b, j])[0]) if (n_out == 2 and b == 0 and j == 0) else None
                pairs[b, j] = draw_pairs(rng, N, pairs_spec[1], hit)

    out = dict(proj=proj32, pts=pts32, pairs=pairs, outlier=outlier)
    x_dlt = np.zeros((B, J, 3))
    x_ref = np.zeros((B, J, 3))
    xstar = np.zeros((B, J, 3))
    inliers = np.zeros((B, J, N), bool)
    ref_cost = np.zeros((B, J))
    slack = np.zeros((B, J))
    hyp_margin, sv_gap = np.inf, np.inf
    for b in range(B):
        for j in range(J):
            pl = pairs if pairs.ndim == 2 else pairs[b, j]
            P, x2d = proj[b], pts[b, :, j]
            x0, inl0 = reference_ransac(net, P, x2d, pl, False)
            x1, inl1 = reference_ransac(net, P, x2d, pl, True)
            assert np.array_equal(inl0, inl1)
            x_dlt[b, j], x_ref[b, j] = x0, x1
            inliers[b, j, inl0] = True
            # decidability of every hypothesis of this point
            for a, c in pl:
                A = np.zeros((4, 4))
                for r, v in enumerate((a, c)):
                    A[2 * r] = x2d[v, 0] * P[v, 2] - P[v, 0]
                    A[2 * r + 1] = x2d[v, 1] * P[v, 2] - P[v, 1]
                s = np.linalg.svd(A, compute_uv=False)
                sv_gap = min(sv_gap, (s[2] - s[3]) / s[0])
                xh = multiview.triangulate_point_from_multiple_views_linear(P[[a, c]], x2d[[a, c]])
                err = multiview.calc_reprojection_error_matrix(np.array([xh]), x2d, P)[0]
                rest = [v for v in range(N) if v not in (a, c)]
                if rest:
                    hyp_margin = min(hyp_margin, np.abs(err[rest] - EPSILON).min())
            s = np.linalg.svd(np.concatenate([np.stack([x2d[v, 0] * P[v, 2] - P[v, 0], x2d[v, 1] * P[v, 2] - P[v, 1]])
                                             for v in inl0]), compute_uv=False)
            sv_gap = min(sv_gap, (s[2] - s[3]) / s[0])
            # polished minimiser over the inlier views
            Pi, xi = P[inl0], x2d[inl0]

            def fun(x):
                return multiview.calc_reprojection_error_matrix(np.array([x]), xi, Pi)[0]
            tight = least_squares(fun, x0, loss="huber", method="trf", ftol=1e-15, xtol=1e-15, gtol=1e-15).x
            cands = [tight, polish(tight, Pi, xi), polish(x1, Pi, xi)]
            best = min(cands, key=lambda x: cost(x, Pi, xi))
            ref_cost[b, j] = cost(x1, Pi, xi)
            assert cost(best, Pi, xi) <= min(ref_cost[b, j], cost(tight, Pi, xi))
            assert abs(0.5 * np.sum(np.where(fun(x1) ** 2 <= 1, fun(x1) ** 2, 2 * fun(x1) - 1)) - ref_cost[b, j]) \
                <= 1e-12 * max(1.0, ref_cost[b, j])          # `cost` restates the reference's cost
            xstar[b, j] = best
            slack[b, j] = f32_neighbour_slack(best, Pi, xi)
    assert hyp_margin > 1e-3, (name, hyp_margin)
    assert sv_gap > 1e-6, (name, sv_gap)
    # the reference's reprojection-error matrix at its DLT points, per frame: (J, N)
    err = np.stack([multiview.calc_reprojection_error_matrix(x_dlt[b], pts[b], proj[b]) for b in range(B)])
    out.update(x_dlt=x_dlt, x_ref=x_ref, xstar=xstar, inliers=inliers, ref_cost=ref_cost, cost_slack=slack,
               err_dlt=err)
    d = np.linalg.norm(x_ref - xstar, axis=-1)
    print(f"{name:14s} B={B} N={N} J={J:2d} pairs={pairs.shape}  inlier counts {sorted(set(inliers.sum(-1).ravel()))}  "
          f"|x_ref - x*| mm: median {np.median(d):.3g}  max {d.max():.3g}   "
          f"epsilon margin {hyp_margin:.3g}  sv gap {sv_gap:.3g}  f32 slack max {slack.max():.3g}")
    return out


def main():
    net, multiview = import_reference()
    data = dict(cases=np.array([c[0] for c in CASES]), epsilon=np.array(EPSILON))
    for k, (name, B, N, J, n_out, spec) in enumerate(CASES):
        for key, val in capture(net, multiview, name, B, N, J, n_out, spec, seed=100 + k).items():
            data[f"{name}.{key}"] = val
    path = os.path.join(HERE, "ransac.npz")
    np.savez_compressed(path, **data)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
