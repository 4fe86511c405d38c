"""The DLT null-vector solver (csrc/dlt_solver.hpp) on systems with known answers: every path
(zero column, inverse iteration early and late, the inertia check, the Jacobi SVD and its
choice of column), through mvn_dlt, the RANSAC kernel and the backward kernel.

The systems and the proof that they are what they claim are in dlt_solver_model.py and
test_dlt_solver_model.py (no GPU); mvn_debug_dlt_trace reports the path each point took, and
its point is asserted bit-equal to mvn_dlt's wherever it is used.
"""
import functools

import numpy as np
import pytest
import torch

import dlt_solver_model as m
from conftest import assert_bits_equal, max_rel
from oracle import restate_np, restate_torch

pytestmark = pytest.mark.gpu


def _t(a, device):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)


def _dlt(device, proj, pts, conf=None):
    from mvn_rocm import multiview
    return multiview.triangulate_batch_of_points(_t(proj, device), _t(pts, device), _t(conf, device)).cpu().numpy()


def _trace(device, proj, pts, conf=None):
    """(xyz (B, J, 3), path (B, J), steps (B, J)) of mvn_debug_dlt_trace; xyz is checked against
    mvn_dlt's bits."""
    from mvn_rocm import _lib
    P, p, c = _t(proj, device), _t(pts, device), _t(conf, device)
    B, N, J = p.shape[:3]
    xyz = torch.empty((B, J, 3), dtype=torch.float32, device=device)
    path = torch.full((B, J), -1, dtype=torch.int32, device=device)
    steps = torch.full((B, J), -1, dtype=torch.int32, device=device)
    code = _lib.load().mvn_debug_dlt_trace(P.data_ptr(), p.data_ptr(), None if c is None else c.data_ptr(),
                                           xyz.data_ptr(), path.data_ptr(), steps.data_ptr(), B, N, J,
                                           torch.cuda.current_stream().cuda_stream)
    _lib.check(code, "mvn_debug_dlt_trace")
    xyz = xyz.cpu().numpy()
    assert_bits_equal(xyz, _dlt(device, proj, pts, conf))
    return xyz, path.cpu().numpy(), steps.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _exact(n_views):
    return m.batch(n_views)


def _ulps(got, want):
    """Distance in f32 ulps between same-signed finite values (as ordered integers)."""
    a = np.float32(got).view(np.int32).astype(np.int64)
    b = np.float32(want).view(np.int32).astype(np.int64)
    return np.abs(a - b)


def _closed_form_errors(got, expect, name):
    """The solver stops within 1e-10 of the null vector, far inside half an f32 ulp: a dyadic
    coordinate must come out bit-equal, any other within one ulp of float32(closed form).
    Returns the coordinates that miss, as messages."""
    bad = []
    for i, fr in enumerate(expect):
        want = np.float32(float(fr))
        if m.is_dyadic(fr):
            ok = np.float32(got[i]).view(np.uint32) == want.view(np.uint32)
        else:
            ok = np.isfinite(got[i]) and np.sign(got[i]) == np.sign(want) and _ulps(got[i], want) <= 1
        if not ok:
            bad.append(f"{name}: coordinate {i} is {got[i]!r}, closed form {want!r}")
    return bad


# ----------------------------------------------------------------------------- forward, exact data
@pytest.mark.parametrize("n_views", (2, 4))
def test_exact_systems_take_their_path_and_return_the_closed_form(device, n_views):
    names, kinds, proj, pts, A, expect = _exact(n_views)
    xyz, path, steps = _trace(device, proj, pts)
    print("path / steps:", {n: (int(p), int(s)) for n, p, s in zip(names, path[:, 0], steps[:, 0])})
    bad = []                                                  # every miss of the batch, not the first
    for i, (name, kind) in enumerate(zip(names, kinds)):
        p, s, got = int(path[i, 0]), int(steps[i, 0]), xyz[i, 0]
        if kind == "tied":
            # any vector of the tied pair's span: |A X| / |X| = sigma_min (the next one is 8 / 3 of it)
            sv = np.linalg.svd(A[i].astype(np.float64), compute_uv=False)
            X = np.append(got.astype(np.float64), 1.0)
            res = np.linalg.norm(A[i] @ X) / np.linalg.norm(X)
            if not (np.isfinite(got).all() and abs(res - sv[3]) <= 1e-6 * sv[3]):   # no tied column has X[3] = 0
                bad.append(f"{name}: {got} has residual {res}, sigma_min {sv[3]}")
            continue
        if kind == "pivot0":
            # (-q / p, 0, 0): the zeros may come out as +-0 or rounding-level numbers
            if not np.abs(got - np.array([float(f) for f in expect[i]])).max() <= 1e-10:
                bad.append(f"{name}: {got}, closed form {[float(f) for f in expect[i]]}")
        else:
            bad += _closed_form_errors(got, expect[i], name)
        if kind in ("jacobi", "ortho"):
            ok = p == m.PATH_JACOBI and 2 <= s <= 40
        elif kind in ("rank3", "pivot0"):
            ok = p == m.PATH_INVERSE_ITERATION and 2 <= s <= 3
        else:
            assert kind == "late"
            ok = p == m.PATH_JACOBI or (p == m.PATH_INVERSE_ITERATION and 9 <= s <= 12)
        if not ok:
            bad.append(f"{name}: path {p}, steps {s}")
    assert not bad, "\n".join(bad)


def test_jacobi_returns_each_of_its_four_columns(device):
    """The rotations of (16, 8, 3, 2) with Q2 put the smallest singular value, and after the
    Jacobi sweeps the smallest column (kmin), at each of the four positions: four different
    closed-form points, all on the Jacobi path."""
    names, kinds, proj, pts, _, expect = _exact(2)
    rows = [names.index(f"jacobi-q2-{s}-n2") for s in ("2_16_8_3", "3_2_16_8", "8_3_2_16", "16_8_3_2")]
    assert len({tuple(expect[i]) for i in rows}) == 4
    xyz, path, _ = _trace(device, proj[rows], pts[rows])
    assert (path == m.PATH_JACOBI).all()
    bad = [e for r, i in enumerate(rows) for e in _closed_form_errors(xyz[r, 0], expect[i], names[i])]
    assert not bad, "\n".join(bad)


# ----------------------------------------------------------------------------- one wave, three paths
def _mixed(n_special):
    """96 four-view points with one joint each (two waves, the second half full): ordinary
    synthetic joints, and, with n_special, exact Jacobi / orthogonal-start / rank-3 systems and
    a zero-confidence joint among them.  Returns proj, pts, conf, {index: name}."""
    from mvn_rocm import synth
    ab = synth.algebraic_batch(96, 4, 1, seed=5)
    proj, pts, conf = ab.proj.numpy().copy(), ab.points.numpy().copy(), ab.confidences.numpy().copy()
    names, _, eproj, epts, _, _ = _exact(4)
    special = {3: "jacobi-q1-16_8_3_2-n4", 5: "ortho-h-8_4_2_1-n4", 17: "jacobi-q2-3_2_16_8-n4", 30: "rank3-q1-8_4_2_0-n4",
               31: "pivot0-2_1-n4", 62: "ortho-q1-3_2_16_8-n4", 63: "late-q1-16_8_3_1-n4", 70: "jacobi-q2-16_8_2_5-n4"}
    if not n_special:
        return proj, pts, conf, {}
    for at, name in special.items():
        i = names.index(name)
        proj[at], pts[at], conf[at] = eproj[i], epts[i], 1.0
    conf[9] = 0.0                                             # A = 0: the zero-column path, (0, 0, 0)
    special[9] = "zero-confidence"
    return proj, pts, conf, special


def test_lanes_on_three_paths_do_not_disturb_each_other(device):
    plain = _dlt(device, *_mixed(False)[:3])
    proj, pts, conf, special = _mixed(True)
    xyz, path, steps = _trace(device, proj, pts, conf)
    ordinary = np.array([i not in special for i in range(96)])
    assert_bits_equal(xyz[ordinary], plain[ordinary])
    assert (path[ordinary] == m.PATH_INVERSE_ITERATION).all()
    print("steps of the ordinary joints:", np.bincount(steps[ordinary].ravel()).tolist())
    assert max_rel(plain, restate_np.triangulate_batch_of_points(*_mixed(False)[:3])) <= 1e-6
    assert path[9, 0] == m.PATH_ZERO_COLUMN and steps[9, 0] == 0
    assert_bits_equal(xyz[9, 0], np.zeros(3, np.float32))
    assert set(path[:64, 0].tolist()) == {0, 1, 2}            # all three in the first wave
    names, _, _, _, _, expect = _exact(4)
    alone = _dlt(device, *_exact(4)[2:4])
    for at, name in special.items():
        if at != 9:
            assert_bits_equal(xyz[at, 0], alone[names.index(name), 0])       # nor do the special ones mind their wave


def test_non_finite_points_stay_in_their_lane(device):
    """A NaN pixel and an infinite pixel among the mixed batch: the call returns, every other
    joint keeps its bits, the NaN joint is NaN (the device-assertion build counts nothing: the
    conftest fixture checks after every GPU test)."""
    proj, pts, conf, special = _mixed(True)
    clean = _dlt(device, proj, pts, conf)
    pts = pts.copy()
    pts[40, 1, 0, 0] = np.nan
    pts[41, 2, 0, 1] = np.inf
    xyz, path, _ = _trace(device, proj, pts, conf)
    others = np.array([i not in (40, 41) for i in range(96)])
    assert_bits_equal(xyz[others], clean[others])
    assert np.isnan(xyz[40]).all()


# ----------------------------------------------------------------------------- scaling
def _scaling_rows():
    names = _exact(2)[0]
    return [names.index(f"{k}-{q}-{s}-n2") for q in ("q1", "q2") for k, s in (("jacobi", "16_8_3_2"), ("late", "16_8_3_1"))]


@pytest.mark.parametrize("n_views", (2, 4))
def test_power_of_two_confidences_change_no_bit(device, n_views):
    """All confidences 2^k, k = +-20 and +-60: the rows are normal f32 numbers and exactly 2^k A.
    Every quantity of the solver then scales by a power of four or of two, which the Newton-
    refined reciprocal estimates follow exactly, and every threshold is relative: the same path,
    steps and bits as k = 0."""
    names, _, proj, pts, _, expect = _exact(n_views)
    rows = [names.index(names[i].replace("-n2", f"-n{n_views}")) for i in _scaling_rows()]
    base = _trace(device, proj[rows], pts[rows])
    bad = [e for r, i in enumerate(rows) for e in _closed_form_errors(base[0][r, 0], expect[i], names[i])]
    assert not bad, "\n".join(bad)
    for k in (-60, -20, 20, 60):
        conf = np.full((len(rows), n_views, 1), 2.0 ** k, np.float32)
        xyz, path, steps = _trace(device, proj[rows], pts[rows], conf)
        assert_bits_equal(xyz, base[0])
        assert np.array_equal(path, base[1]) and np.array_equal(steps, base[2]), k


def test_subnormal_rows(device):
    """Confidences 2^-140: every non-zero entry of the f32 design matrix is subnormal (and still
    exact).  The restatement keeps subnormals; so must the kernel's three f32 operations."""
    names, kinds, proj, pts, _, _ = _exact(2)
    rows = [i for i, k in enumerate(kinds) if k in ("jacobi", "late", "ortho")]
    conf = np.full((len(rows), 2, 1), 2.0 ** -140, np.float32)
    ref = restate_np.triangulate_batch_of_points(proj[rows], pts[rows], conf)
    assert np.isfinite(ref).all()
    xyz, _, _ = _trace(device, proj[rows], pts[rows], conf)
    assert max_rel(xyz, ref) <= 1e-6


# ----------------------------------------------------------------------------- physical cameras
def test_near_coincident_cameras(device):
    """Two pinhole views 0.05 mm apart, a point 3 m away, 5 px of noise: sigma_3 / sigma_4 from
    2.2 to 7.6, non-lattice data on the late steps and on the fallback."""
    proj, pts = m.near_coincident_batch()
    ref = restate_np.triangulate_batch_of_points(proj, pts)
    xyz, path, steps = _trace(device, proj, pts)
    print("path / steps:", dict(zip(m.NEAR_SEEDS, zip(path[:, 0].tolist(), steps[:, 0].tolist()))))
    for i, seed in enumerate(m.NEAR_SEEDS):
        assert max_rel(xyz[i], ref[i]) <= 1e-6, (seed, xyz[i], ref[i])
        if seed in m.NEAR_JACOBI_SEEDS:
            assert path[i, 0] == m.PATH_JACOBI, (seed, path[i, 0], steps[i, 0])
    assert path[m.NEAR_SEEDS.index(1), 0] == m.PATH_INVERSE_ITERATION and 7 <= steps[m.NEAR_SEEDS.index(1), 0] <= 9


# ----------------------------------------------------------------------------- RANSAC's use of the solver
@pytest.mark.parametrize("n_views", (2, 4))
def test_ransac_solves_the_same_systems_to_the_same_bits(device, n_views):
    """No refinement, every view an inlier: the kernel's last solve folds the same integer rows
    (its f64 product and difference are exact here) in the same order as mvn_dlt, so the points
    are mvn_dlt's bits on every path, the Jacobi and the orthogonal-start systems included."""
    from mvn_rocm import multiview
    names, kinds, proj, pts, _, _ = _exact(n_views)
    assert {"jacobi", "ortho", "late", "rank3", "pivot0", "tied"} <= set(kinds)
    want = _dlt(device, proj, pts)
    pairs = torch.tensor([[0, 1]], dtype=torch.int32, device=device) if n_views == 2 else "all"
    xyz, inliers = multiview.triangulate_ransac_batch(_t(proj, device), _t(pts, device), view_pairs=pairs,
                                                      reprojection_error_epsilon=1e30, direct_optimization=False)
    assert inliers.all()
    assert_bits_equal(xyz.cpu().numpy(), want)


# ----------------------------------------------------------------------------- backward
@functools.lru_cache(maxsize=None)
def _backward_case(n_views, use_conf):
    names, _, proj, pts, _, _ = _exact(n_views)
    keep = [names.index(name) for name in m.backward_names(n_views)]
    conf = np.tile(m.backward_conf(n_views)[None, :, None], (len(keep), 1, 1)) if use_conf else None
    gout = np.stack([m.BACKWARD_GOUT[i % 3] for i in range(len(keep))])[:, None, :]
    ref = restate_torch.triangulate_batch_of_points_f32_design(
        torch.from_numpy(proj[keep]), torch.from_numpy(pts[keep]), None if conf is None else torch.from_numpy(conf),
        torch.from_numpy(gout))
    return proj[keep], pts[keep], conf, gout, [r.numpy() for r in ref]


@pytest.mark.parametrize("use_conf", (False, True))
@pytest.mark.parametrize("n_views", (2, 4))
def test_backward_on_close_singular_values(device, n_views, use_conf):
    """mvn_dlt_backward (its own Givens fold and Jacobi SVD) where sigma_3 / sigma_4 is 1.25 to 3
    and 1 / (lambda_4 - lambda_k) is large, against float64 SVD autograd on the identical A
    (the two float64 references agree to 1e-9: test_dlt_solver_model.py)."""
    from mvn_rocm import multiview
    proj, pts, conf, gout, (ref_x, ref_gp, ref_gc) = _backward_case(n_views, use_conf)
    p = _t(pts, device).requires_grad_(True)
    c = _t(conf if use_conf else np.ones(pts.shape[:3], np.float32), device).requires_grad_(True)
    out = multiview.triangulate_batch_of_points(_t(proj, device), p, c)
    assert max_rel(out.detach().cpu().numpy(), ref_x) <= 1e-6
    out.backward(_t(gout, device))
    cf = conf if use_conf else np.ones(pts.shape[:3], np.float32)
    for b in range(len(proj)):                               # per system: their gradients differ by decades
        assert max_rel(p.grad[b].cpu().numpy(), ref_gp[b]) <= 1e-5, b
        # dL/dc_v sums terms of the size of dL/dpt_{v,r} pt_{v,r} / c_v, and for two of the two-view
        # systems they cancel to exactly zero: the error is measured against the larger of the two
        scale = max(np.abs(ref_gc[b]).max(), (np.abs(ref_gp[b]) * np.abs(pts[b]) / cf[b][..., None]).max())
        assert np.abs(c.grad[b].cpu().numpy() - ref_gc[b]).max() <= 1e-5 * scale, (b, scale)
