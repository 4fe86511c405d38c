"""Host side of the RANSAC triangulation and the reprojection error -- no GPU needed: the C ABI's
argument checks return before any HIP call, the Python wrappers assert what the reference
asserts, and the custom ops trace under fake tensors."""
import ctypes

import numpy as np
import pytest
import torch
from torch.fx.experimental.proxy_tensor import make_fx

ARG, SHAPE = -1, -2


@pytest.fixture(scope="module")
def lib():
    from mvn_rocm import _lib
    return _lib.load()


def _ransac(lib, **kw):
    a = dict(proj=1, pts=1, pairs=1, pairs_per_point=0, n_iters=10, epsilon=15.0, direct=1, out_xyz=1,
             out_inliers=1, out_error_mean=None, B=2, N=4, J=17)
    a.update(kw)
    return lib.mvn_triangulate_ransac(a["proj"], a["pts"], a["pairs"], a["pairs_per_point"], a["n_iters"],
                                      a["epsilon"], a["direct"], a["out_xyz"], a["out_inliers"],
                                      a["out_error_mean"], a["B"], a["N"], a["J"], None)


@pytest.mark.parametrize("name", ["proj", "pts", "pairs", "out_xyz", "out_inliers"])
def test_ransac_null_pointers(lib, name):
    assert _ransac(lib, **{name: None}) == ARG


@pytest.mark.parametrize("kw", [dict(pairs_per_point=2), dict(pairs_per_point=-1), dict(direct=2), dict(direct=-1)])
def test_ransac_bad_flags(lib, kw):
    assert _ransac(lib, **kw) == ARG


@pytest.mark.parametrize("kw", [dict(N=1), dict(N=0), dict(N=33), dict(n_iters=0), dict(n_iters=-3), dict(n_iters=4097),
                                dict(B=0), dict(J=0), dict(B=-1), dict(B=1 << 16, J=1 << 15)])
def test_ransac_bad_shapes(lib, kw):
    assert _ransac(lib, **kw) == SHAPE


def test_reprojection_error_argument_checks(lib):
    f = lib.mvn_reprojection_error
    for k in range(4):
        ptrs = [1, 1, 1, 1]
        ptrs[k] = None
        assert f(*ptrs, 2, 4, 17, None) == ARG
    assert f(1, 1, 1, 1, 0, 4, 17, None) == SHAPE
    assert f(1, 1, 1, 1, 2, 0, 17, None) == SHAPE
    assert f(1, 1, 1, 1, 2, 4, -1, None) == SHAPE
    assert f(1, 1, 1, 1, 1 << 16, 4, 1 << 15, None) == SHAPE


def test_header_declares_and_library_exports_the_entry_points(lib):
    import os
    from conftest import ROOT
    from mvn_rocm import _lib
    header = open(os.path.join(ROOT, "include", "mvn_hip.h")).read()
    for name in ("mvn_triangulate_ransac", "mvn_reprojection_error"):
        assert f"int {name}(" in header
        assert name in _lib.SIGNATURES
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr)


def test_wrappers_assert_what_the_reference_asserts():
    from mvn_rocm import multiview
    proj, pts = torch.randn(2, 4, 3, 4), torch.randn(2, 3, 5, 2)
    with pytest.raises(AssertionError):                      # triangulation.py:73
        multiview.triangulate_ransac_batch(proj, pts)
    with pytest.raises(AssertionError):                      # triangulation.py:74
        multiview.triangulate_ransac_batch(proj[:, :1], pts[:, :1])
    with pytest.raises(AssertionError):
        multiview.triangulate_ransac(np.zeros((4, 3, 4)), np.zeros((3, 2)))
    with pytest.raises(AssertionError):
        multiview.triangulate_ransac(np.zeros((1, 3, 4)), np.zeros((1, 2)))
    with pytest.raises(AssertionError):
        multiview.calc_reprojection_error_matrix(torch.randn(5, 3), torch.randn(3, 5, 2), torch.randn(4, 3, 4))


def test_wrappers_refuse_what_the_kernel_cannot_take():
    from mvn_rocm import multiview
    proj, pts = torch.randn(1, 4, 3, 4), torch.randn(1, 4, 5, 2)
    with pytest.raises(ValueError):
        multiview.triangulate_ransac_batch(torch.randn(1, 33, 3, 4), torch.randn(1, 33, 5, 2))
    with pytest.raises(ValueError):
        multiview.triangulate_ransac_batch(proj, pts, view_pairs="sometimes")
    with pytest.raises(ValueError):
        multiview.triangulate_ransac_batch(proj, pts, view_pairs="random", n_iters=0)
    with pytest.raises(TypeError):
        multiview.triangulate_ransac_batch(proj, pts, view_pairs=torch.zeros(3, 2))
    with pytest.raises(ValueError):
        multiview.triangulate_ransac_batch(proj, pts, view_pairs=torch.zeros(2, 5, 3, 2, dtype=torch.int64))
    with pytest.raises(ValueError):
        multiview.triangulate_ransac_batch(proj, pts, view_pairs=torch.zeros(3, 3, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        multiview.triangulate_ransac_batch(proj, pts)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        multiview.calc_reprojection_error_matrix(torch.randn(5, 3), pts[0], proj[0])


def test_all_view_pairs_are_lexicographic():
    import itertools
    from mvn_rocm import multiview
    for n in (2, 5, 8):
        p = multiview.all_view_pairs(n)
        assert p.dtype == torch.int32
        assert p.tolist() == [list(q) for q in itertools.combinations(range(n), 2)]


def test_random_view_pairs_on_the_host_generator():
    from mvn_rocm import multiview
    g = torch.Generator().manual_seed(3)
    p = multiview.random_view_pairs(2, 3, 5, 40, "cpu", g)
    assert tuple(p.shape) == (2, 3, 40, 2) and p.dtype == torch.int32
    assert bool(((p >= 0) & (p < 5)).all()) and bool((p[..., 0] < p[..., 1]).all())
    assert len({tuple(q) for q in p.reshape(-1, 2).tolist()}) == 10
    assert torch.equal(p, multiview.random_view_pairs(2, 3, 5, 40, "cpu", torch.Generator().manual_seed(3)))


def _targets(gm):
    return {str(n.target) for n in gm.graph.nodes if n.op == "call_function"}


def test_custom_ops_trace_under_fake_tensors():
    from mvn_rocm import multiview
    B, N, J = 2, 4, 5
    proj, pts = torch.randn(B, N, 3, 4), torch.randn(B, N, J, 2)

    def ransac(proj, pts, pairs):
        return multiview.triangulate_ransac_batch(proj, pts, view_pairs=pairs, return_error=True)

    for pairs in (torch.zeros(7, 2, dtype=torch.int64), torch.zeros(B, J, 7, 2, dtype=torch.int32)):
        gm = make_fx(ransac, tracing_mode="fake")(proj, pts, pairs)
        assert "mvn_rocm.ransac.default" in _targets(gm)
        out = [n for n in gm.graph.nodes if n.op == "output"][0].args[0]
        xyz, inliers, err = (n.meta["val"] for n in out)
        assert (tuple(xyz.shape), xyz.dtype) == ((B, J, 3), torch.float32)
        assert (tuple(inliers.shape), inliers.dtype) == ((B, J, N), torch.bool)
        assert (tuple(err.shape), err.dtype) == ((B, J), torch.float32)
    gm = make_fx(lambda p, x: multiview.triangulate_ransac_batch(p, x), tracing_mode="fake")(proj, pts)   # 'all'
    assert "mvn_rocm.ransac.default" in _targets(gm)

    X = torch.randn(B, J, 3)
    gm = make_fx(lambda X, x, p: multiview.calc_reprojection_error_matrix(X, x, p), tracing_mode="fake")(X, pts, proj)
    assert "mvn_rocm.reprojection_error.default" in _targets(gm)
    val = [n for n in gm.graph.nodes if n.op == "output"][0].args[0].meta["val"]
    assert (tuple(val.shape), val.dtype) == ((B, J, N), torch.float32)
    gm = make_fx(lambda X, x, p: multiview.calc_reprojection_error_matrix(X, x, p), tracing_mode="fake")(X[0], pts[0], proj[0])
    val = [n for n in gm.graph.nodes if n.op == "output"][0].args[0].meta["val"]
    assert tuple(val.shape) == (J, N)
