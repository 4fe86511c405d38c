"""Guards of the DLT solver tests, no GPU: every system test_gpu_dlt_solver.py feeds the kernels
is what it claims to be.  The f32 design matrix is the intended integer matrix, float64 LAPACK
reproduces the closed-form point, and the NumPy model of the solver (dlt_solver_model.py) takes
the path the case is built for."""
import numpy as np
import pytest
import torch

import dlt_solver_model as m
from oracle import restate_np, restate_torch


def _float(fr):
    return np.array([float(f) for f in fr])


@pytest.fixture(scope="module", params=(2, 4))
def exact(request):
    return m.batch(request.param)


def test_case_list_covers_the_table(exact):
    names, kinds = exact[0], exact[1]
    assert len(set(names)) == len(names)
    assert {k: kinds.count(k) for k in set(kinds)} == {"jacobi": 14, "late": 6, "rank3": 4, "tied": 2, "ortho": 5,
                                                         "pivot0": 2}


def test_f32_design_matrix_is_the_integer_matrix(exact):
    """The three f32 operations of multiview.py:150-152 are exact on the affine cameras."""
    _, _, proj, pts, A, _ = exact
    assert np.abs(A).max() < 128
    for i in range(len(A)):
        got = restate_np.design_matrix(proj[i], pts[i, :, 0], None)
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.int64), A[i]) and np.array_equal(got, A[i])


def test_lapack_reproduces_the_closed_form(exact):
    names, kinds, proj, pts, A, expect = exact
    ref = restate_np.triangulate_batch_of_points(proj, pts)[:, 0]
    for i, kind in enumerate(kinds):
        sv = np.linalg.svd(A[i].astype(np.float64), compute_uv=False)
        if kind == "tied":
            assert abs(sv[2] / sv[3] - 1.0) < 1e-14, names[i]
            continue
        assert sv[2] > 1.1 * sv[3], names[i]
        assert np.abs(ref[i] - _float(expect[i])).max() <= 1e-13, names[i]


def test_model_takes_the_intended_path(exact):
    names, kinds, _, _, A, expect = exact
    for i, kind in enumerate(kinds):
        X, path, steps = m.solve(A[i])
        err = np.abs(m.point(X) - _float(expect[i])).max()
        if kind == "jacobi":
            assert (path, steps) == (m.PATH_JACOBI, 12) and err <= 1e-13, (names[i], path, steps, err)
        elif kind == "late":
            assert path == m.PATH_JACOBI or (path == m.PATH_INVERSE_ITERATION and steps >= 9), (names[i], path, steps)
            assert err <= 1e-10, (names[i], err)
        elif kind == "rank3":
            assert (path, steps) == (m.PATH_INVERSE_ITERATION, 2) and err <= 1e-14, (names[i], path, steps, err)
            R = m.fold(A[i])
            d = np.abs(np.diag(R))
            assert (d <= 1e-13 * d.max()).any() and (d > 1e-30 * d.max()).all(), names[i]   # tiny, above the guard
        elif kind == "pivot0":
            assert (path, steps) == (m.PATH_INVERSE_ITERATION, 2) and err <= 1e-15, (names[i], path, steps, err)
        elif kind == "ortho":
            assert path == m.PATH_JACOBI and err <= 1e-13, (names[i], path, err)
    assert any(k == "late" and m.solve(a)[1] == m.PATH_INVERSE_ITERATION for k, a in zip(kinds, A))


def test_model_without_the_inertia_check_returns_another_singular_vector(exact):
    """What the 'ortho' systems are for: inverse iteration alone reports convergence on a
    singular vector that is not the smallest one's, a finite, plausible, wrong point."""
    names, kinds, _, _, A, expect = exact
    for i, kind in enumerate(kinds):
        X, path, steps = m.solve(A[i], check=False)
        if kind == "ortho":
            assert path == m.PATH_INVERSE_ITERATION, names[i]
            assert np.abs(m.point(X) - _float(expect[i])).max() > 0.3, names[i]
            assert np.isfinite(m.point(X)).all()
        elif kind != "tied":
            assert np.abs(m.point(X) - _float(expect[i])).max() <= 1e-10, names[i]
            assert path == m.solve(A[i])[1], names[i]         # the check changes no other case's path
    # the orthogonality that causes it, in integers
    for name, kind, Q, s in m.spectral_cases(2):
        if kind == "ortho":
            assert Q[:, int(np.argmin(s))].sum() == 0, name


def test_pivot_guard_is_what_keeps_the_zero_pivot_systems_on_inverse_iteration(exact):
    """'pivot0': R[3][3] is exactly zero and column 3 is not.  Without the guard the reciprocal is
    infinite, the first step is NaN and the point goes to the Jacobi SVD (which is right too:
    only the trace sees the guard)."""
    names, kinds, _, _, A, _ = exact
    for i, kind in enumerate(kinds):
        if kind == "pivot0":
            R = m.fold(A[i])
            assert R[3, 3] == 0.0 and R[0, 3] != 0.0 and np.diag(R)[:3].all(), names[i]
            ok, x, steps = m.inverse_iteration(R, pivot_guard=False)
            assert not ok and steps == 1 and np.isnan(x).any(), names[i]


def test_scaled_systems_stay_normal_and_exact():
    """Confidences 2^k, k = +-20, +-60: rows are normal f32 numbers, exactly 2^k A, and the model
    returns identical bits; 2^-140 makes every non-zero entry subnormal and is still exact."""
    _, kinds, proj, pts, A, _ = m.batch(2, ("jacobi", "late"))
    for k in (-60, -20, 20, 60, -140):
        conf = np.full(2, 2.0 ** k, np.float32)
        for i in range(len(A)):
            got = restate_np.design_matrix(proj[i], pts[i, :, 0], conf)
            assert np.array_equal(got.astype(np.float64), A[i] * 2.0 ** k)
            nz = np.abs(got[got != 0])
            assert (nz < np.finfo(np.float32).tiny).all() if k == -140 else (nz >= np.finfo(np.float32).tiny).all()
            if k != -140:
                X0, p0, s0 = m.solve(A[i].astype(np.float64))
                X1, p1, s1 = m.solve(got.astype(np.float64))
                assert (p0, s0) == (p1, s1) and np.array_equal(X0, X1)


def test_near_coincident_cameras_are_ill_conditioned_and_the_model_meets_the_bar():
    proj, pts = m.near_coincident_batch()
    ref = restate_np.triangulate_batch_of_points(proj, pts)[:, 0]
    paths = {}
    for i, seed in enumerate(m.NEAR_SEEDS):
        A = restate_np.design_matrix(proj[i], pts[i, :, 0], None).astype(np.float64)
        X, path, steps = m.solve(A)
        paths[seed] = (path, steps)
        assert m.sigma_ratio(A) < 8.0
        assert np.abs(m.point(X) - ref[i]).max() / np.abs(ref[i]).max() <= 1e-6, seed
    for seed in m.NEAR_JACOBI_SEEDS:
        assert paths[seed][0] == m.PATH_JACOBI, (seed, paths)
    assert paths[1] == (m.PATH_INVERSE_ITERATION, 8) and paths[2] == (m.PATH_INVERSE_ITERATION, 12), paths


@pytest.mark.parametrize("use_conf", (False, True))
def test_backward_reference_agrees_with_the_closed_form(exact, use_conf):
    """The float64 SVD autograd the GPU test compares against, and numpy's evaluation of the
    closed form in backward.hip's header comment, agree to 1e-9 on every case the GPU test
    uses: the gradient is well-posed there."""
    names, kinds, proj, pts, A, _ = exact
    n = proj.shape[1]
    keep = [names.index(name) for name in m.backward_names(n)]
    assert len(keep) == 23
    conf = np.tile(m.backward_conf(n)[None, :, None], (len(keep), 1, 1)) if use_conf else None
    gout = np.stack([m.BACKWARD_GOUT[i % 3] for i in range(len(keep))])[:, None, :]
    _, gp, gc = restate_torch.triangulate_batch_of_points_f32_design(
        torch.from_numpy(proj[keep]), torch.from_numpy(pts[keep]), None if conf is None else torch.from_numpy(conf),
        torch.from_numpy(gout))
    for r, i in enumerate(keep):
        c = conf[r, :, 0] if use_conf else np.ones(n)
        gp2, gc2 = m.backward_closed_form(proj[i], pts[i, :, 0], c, gout[r, 0])
        scale = max(np.abs(gp2).max(), np.abs(gc2).max())
        assert np.abs(gp[r, :, 0].numpy() - gp2).max() <= 1e-9 * scale, names[i]
        assert np.abs(gc[r, :, 0].numpy() - gc2).max() <= 1e-9 * scale, names[i]
