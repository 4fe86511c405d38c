"""RANSAC triangulation with Huber refinement and the batched reprojection error on the GPU,
against the reference's recorded results (tests/golden/ransac.npz, written by
tests/golden/make_golden_ransac.py; nothing here reads the reference or scipy).

Bounds:
  * inlier masks equal the reference's for every point (the capture script asserts that no
    hypothesis's error lies within 1e-3 of epsilon, so they are decidable);
  * unrefined points: max|d| / max|ref| <= 1e-4 against the reference's float64 answer;
  * refined points: the cost 1/2 sum rho(r_v^2) of the returned point does not exceed the
    reference's cost at its own answer plus `cost_slack`, the largest cost change among the
    float32 neighbours of the polished minimiser x* (the output is float32); and
    |x - x*| <= max(1e-4 max|x*|, 2 |x_ref - x*|), both terms from the fixture.
"""
import itertools

import numpy as np
import pytest
import torch

from conftest import assert_bits_equal, load_golden, max_rel

pytestmark = pytest.mark.gpu

G = load_golden("ransac.npz")
CASES = [str(c) for c in G["cases"]]
EPS = float(G["epsilon"])


def case(name):
    return {k.split(".", 1)[1]: v for k, v in G.items() if k.startswith(name + ".")}


def run(device, proj, pts, pairs, direct, **kw):
    from mvn_rocm import multiview
    if not isinstance(pairs, str):
        pairs = torch.as_tensor(pairs).to(device)
    out = multiview.triangulate_ransac_batch(torch.as_tensor(proj).to(device), torch.as_tensor(pts).to(device),
                                             view_pairs=pairs, reprojection_error_epsilon=EPS,
                                             direct_optimization=direct, **kw)
    return tuple(o.cpu().numpy() for o in out)


_results = {}


@pytest.fixture
def result(device):
    """(xyz, inliers, mean error) of a fixture case, computed once per (case, direct)."""
    def get(name, direct):
        if (name, direct) not in _results:
            c = case(name)
            _results[name, direct] = run(device, c["proj"], c["pts"], c["pairs"], direct, return_error=True)
        return _results[name, direct]
    return get


def huber_cost(x, proj, pts):
    """1/2 sum rho(r_v^2): r_v half the pixel distance, rho(z) = z (z <= 1) else 2 sqrt(z) - 1."""
    h = proj[:, :, :3] @ x + proj[:, :, 3]
    z = 0.25 * ((pts - h[:, :2] / h[:, 2:]) ** 2).sum(1)
    return 0.5 * np.where(z <= 1.0, z, 2.0 * np.sqrt(z) - 1.0).sum()


# ------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("direct", [False, True])
@pytest.mark.parametrize("name", CASES)
def test_inlier_masks_equal_the_references(result, name, direct):
    xyz, inliers, _ = result(name, direct)
    ref = case(name)["inliers"]
    assert inliers.dtype == np.bool_ and inliers.shape == ref.shape
    assert np.array_equal(inliers, ref), f"{int((inliers != ref).any(-1).sum())} of {ref[..., 0].size} points differ"


@pytest.mark.parametrize("name", CASES)
def test_unrefined_points_match_the_reference(result, name):
    xyz, _, _ = result(name, False)
    assert xyz.dtype == np.float32
    err = max_rel(xyz, case(name)["x_dlt"])
    print(f"{name}: max-rel {err:.3g}")
    assert err <= 1e-4


@pytest.mark.parametrize("name", CASES)
def test_refined_cost_does_not_exceed_the_references(result, name):
    c = case(name)
    xyz, inliers, _ = result(name, True)
    proj, pts = c["proj"].astype(np.float64), c["pts"].astype(np.float64)
    worst = -np.inf
    for b, j in np.ndindex(*xyz.shape[:2]):
        v = np.nonzero(c["inliers"][b, j])[0]
        cost = huber_cost(xyz[b, j].astype(np.float64), proj[b, v], pts[b, v, j])
        worst = max(worst, cost - c["ref_cost"][b, j] - c["cost_slack"][b, j])
    print(f"{name}: max (cost - reference cost - f32 slack) {worst:.3g}")
    assert worst <= 0.0


@pytest.mark.parametrize("name", CASES)
def test_refined_points_are_as_close_to_the_minimum_as_the_reference(result, name):
    c = case(name)
    xyz, _, _ = result(name, True)
    dist = np.linalg.norm(xyz.astype(np.float64) - c["xstar"], axis=-1)
    bound = np.maximum(1e-4 * np.abs(c["xstar"]).max(), 2.0 * np.linalg.norm(c["x_ref"] - c["xstar"], axis=-1))
    print(f"{name}: max |x - x*| {dist.max():.3g} mm (reference: {np.linalg.norm(c['x_ref'] - c['xstar'], axis=-1).max():.3g} mm)")
    assert (dist <= bound).all(), f"worst excess {(dist - bound).max():.3g} mm"


@pytest.mark.parametrize("name", CASES)
def test_mean_error_is_the_reprojection_error_over_the_inliers(device, result, name):
    from mvn_rocm import multiview
    c = case(name)
    xyz, inliers, mean = result(name, True)
    err = multiview.calc_reprojection_error_matrix(torch.from_numpy(xyz).to(device), torch.from_numpy(c["pts"]).to(device),
                                                   torch.from_numpy(c["proj"]).to(device)).cpu().numpy().astype(np.float64)
    want = (err * inliers).sum(-1) / inliers.sum(-1)
    # each error and the mean are rounded to float32 once: a few 2^-24 relative
    np.testing.assert_allclose(mean, want, rtol=1e-6, atol=0)


@pytest.mark.parametrize("name", CASES)
def test_reprojection_error_matches_the_reference(device, name):
    from mvn_rocm import multiview
    c = case(name)
    X, pts, proj = (torch.from_numpy(np.asarray(a, np.float32)).to(device) for a in (c["x_dlt"], c["pts"], c["proj"]))
    out = multiview.calc_reprojection_error_matrix(X, pts, proj)
    assert out.dtype == torch.float32 and tuple(out.shape) == c["err_dlt"].shape
    assert max_rel(out.cpu().numpy(), c["err_dlt"]) <= 1e-4
    one = multiview.calc_reprojection_error_matrix(X[-1], pts[-1], proj[-1])          # the reference's own form
    assert tuple(one.shape) == c["err_dlt"].shape[1:]
    assert_bits_equal(one.cpu().numpy(), out[-1].cpu().numpy())
    assert max_rel(one.cpu().numpy(), c["err_dlt"][-1]) <= 1e-4


def test_two_calls_are_bit_identical(device):
    c = case("n5_out2")
    a = run(device, c["proj"], c["pts"], c["pairs"], True, return_error=True)
    b = run(device, c["proj"], c["pts"], c["pairs"], True, return_error=True)
    assert_bits_equal(a[0], b[0])
    assert np.array_equal(a[1], b[1])
    assert_bits_equal(a[2], b[2])


# ------------------------------------------------------------------------ selection
def two_cluster_scene():
    """One point seen by six views: views 0-2 see it at A, views 3-5 at B, exactly (no noise).
    A pair inside a cluster has that cluster as its inliers (3); a pair across has only itself (2)."""
    from mvn_rocm import synth
    ab = synth.algebraic_batch(1, 6, 1, seed=9, noise_px=0.0)
    proj = ab.proj.numpy()
    A = ab.points_3d.numpy()[0, 0]
    Bp = A + np.array([600.0, -500.0, 400.0])
    P = proj[0].astype(np.float64)

    def project(X):
        h = P[:, :, :3] @ X + P[:, :, 3]
        return h[:, :2] / h[:, 2:]
    uvA, uvB = project(A), project(Bp)
    # the scene is what it claims: each cluster's point is far outside epsilon in the other's views
    assert (0.5 * np.linalg.norm(uvA - uvB, axis=1) > 2 * EPS).all()
    pts = np.where(np.arange(6)[:, None] < 3, uvA, uvB).astype(np.float32).reshape(1, 6, 1, 2)
    return proj, pts


FIRST, SECOND = [True] * 3 + [False] * 3, [False] * 3 + [True] * 3


def test_ties_resolve_to_the_first_hypothesis(device):
    proj, pts = two_cluster_scene()
    for pairs, want in (([(0, 1), (3, 4)], FIRST), ([(3, 4), (0, 1)], SECOND), ([(0, 3), (4, 5), (1, 2)], SECOND)):
        _, inl = run(device, proj, pts, np.array(pairs, np.int32), False)
        assert inl[0, 0].tolist() == want, pairs


@pytest.mark.parametrize("n_iters", [17, 33])
def test_lane_strided_hypothesis_loop(device, n_iters):
    """More hypotheses than the 16 lanes of a point's group: the entries past 16 are evaluated and
    the (count, lowest index) order holds across lanes and trips."""
    proj, pts = two_cluster_scene()
    weak = [(0, 3)] * n_iters                                    # two inliers each
    for at, want, winner in (
            ({n_iters - 1: (0, 1)}, FIRST, (0, 1)),                              # only the last entry is good
            ({n_iters - 2: (3, 4), n_iters - 1: (0, 1)}, SECOND, (3, 4)),        # tie: lane 15, then lane 0's next trip
            ({n_iters - 2: (0, 1), n_iters - 1: (3, 4)}, FIRST, (0, 1)),
            ({1: (3, 4), 16: (0, 1)}, SECOND, (3, 4)),                           # tie across trips of different lanes
            ({1: (3, 4), 16: (0, 1), 0: (1, 2)}, FIRST, (1, 2))):
        pairs = list(weak)
        for i, p in at.items():
            pairs[i] = p
        xyz, inl = run(device, proj, pts, np.array(pairs, np.int32), True)
        assert inl[0, 0].tolist() == want, at
        only, _ = run(device, proj, pts, np.array([winner], np.int32), True)    # the same set, so the same point
        assert_bits_equal(xyz, only)


# ------------------------------------------------------------------------ hypothesis handling
@pytest.mark.parametrize("bad", [(4, 0), (0, 4), (-1, 2), (2, -1), (1, 1), (2 ** 31 - 1, 0), (-2 ** 31, 1)])
@pytest.mark.parametrize("where", [0, 3, 6])
def test_an_invalid_pair_is_skipped(device, bad, where):
    c = case("n4_shared")                                        # N = 4, six shared pairs
    want = run(device, c["proj"], c["pts"], c["pairs"], True, return_error=True)
    pairs = np.insert(c["pairs"], where, np.array(bad, np.int32), axis=0)
    got = run(device, c["proj"], c["pts"], pairs, True, return_error=True)
    assert np.array_equal(got[1], want[1])
    assert_bits_equal(got[0], want[0])
    assert_bits_equal(got[2], want[2])


def test_only_invalid_pairs_use_all_views(device):
    from mvn_rocm import multiview
    c = case("n4_clean_one")
    pairs = np.array([(4, 0), (1, 1), (-1, 2)], np.int32)
    xyz, inl = run(device, c["proj"], c["pts"], pairs, False)
    assert inl.all()
    # all views, unweighted: the DLT of the same points (float32 rows there, float64 here)
    dlt = multiview.triangulate_batch_of_points(torch.from_numpy(c["proj"]).to(device),
                                                torch.from_numpy(c["pts"]).to(device)).cpu().numpy()
    assert max_rel(xyz, dlt) <= 1e-4


def test_all_pairs_equal_the_explicit_lexicographic_list(device):
    c = case("n8_out3_all")
    explicit = np.array(list(itertools.combinations(range(8), 2)), np.int32)
    assert np.array_equal(explicit, c["pairs"])
    a = run(device, c["proj"], c["pts"], "all", True, return_error=True, n_iters=3)     # n_iters is irrelevant
    b = run(device, c["proj"], c["pts"], explicit, True, return_error=True)
    assert_bits_equal(a[0], b[0])
    assert np.array_equal(a[1], b[1])
    assert_bits_equal(a[2], b[2])


def test_random_pairs_are_reproducible_and_valid(device):
    from mvn_rocm import multiview
    c = case("n5_out2")
    B, N, J = c["pts"].shape[:3]

    def gen():
        return torch.Generator(device=device).manual_seed(1234)
    a = run(device, c["proj"], c["pts"], "random", True, n_iters=24, generator=gen())
    b = run(device, c["proj"], c["pts"], "random", True, n_iters=24, generator=gen())
    assert_bits_equal(a[0], b[0])
    assert np.array_equal(a[1], b[1])
    pairs = multiview.random_view_pairs(B, J, N, 24, device, gen())
    assert pairs.dtype == torch.int32 and tuple(pairs.shape) == (B, J, 24, 2)
    p = pairs.cpu().numpy()
    assert (p >= 0).all() and (p < N).all() and (p[..., 0] < p[..., 1]).all()
    assert len({tuple(q) for q in p.reshape(-1, 2)}) == N * (N - 1) // 2       # every pair is drawn
    e = run(device, c["proj"], c["pts"], p, True)                              # the same draw, explicit
    assert_bits_equal(a[0], e[0])
    assert np.array_equal(a[1], e[1])


# ------------------------------------------------------------------------ layout and dispatch
def test_shared_and_per_point_lists_agree(device):
    c = case("n4_shared")
    B, _, J = c["pts"].shape[:3]
    per_point = np.broadcast_to(c["pairs"], (B, J) + c["pairs"].shape).copy()
    a = run(device, c["proj"], c["pts"], c["pairs"], True, return_error=True)
    b = run(device, c["proj"], c["pts"], per_point, True, return_error=True)
    assert_bits_equal(a[0], b[0])
    assert np.array_equal(a[1], b[1])
    assert_bits_equal(a[2], b[2])


@pytest.mark.parametrize("J", [1, 3, 5])
def test_partially_filled_waves(device, result, J):
    """B J = 1, 3, 5 points: a wave holds four.  Points are independent, so a slice of the batch
    gives the bits the whole batch gives."""
    c = case("n4_out1")
    full = result("n4_out1", True)
    got = run(device, c["proj"][1:], c["pts"][1:, :, 4:4 + J], c["pairs"][1:, 4:4 + J], True, return_error=True)
    assert_bits_equal(got[0], full[0][1:, 4:4 + J])
    assert np.array_equal(got[1], full[1][1:, 4:4 + J])
    assert_bits_equal(got[2], full[2][1:, 4:4 + J])


def test_single_point_form_and_integer_points(device):
    from mvn_rocm import multiview
    c = case("n4_out1")
    proj = torch.from_numpy(c["proj"][0]).to(device)
    pts = torch.from_numpy(c["pts"][0, :, 2]).to(device)
    x, inl = multiview.triangulate_ransac(proj, pts, view_pairs=torch.from_numpy(c["pairs"][0, 2]).to(device))
    full = run(device, c["proj"], c["pts"], c["pairs"], True)
    assert tuple(x.shape) == (3,)
    assert_bits_equal(x.cpu().numpy(), full[0][0, 2])
    assert inl.tolist() == np.nonzero(c["inliers"][0, 2])[0].tolist()
    # integer keypoints (the reference's argmax keypoints) are cast to float32
    ipts = torch.from_numpy(np.rint(c["pts"]).astype(np.int64)).to(device)
    a = multiview.triangulate_ransac_batch(torch.from_numpy(c["proj"]).to(device), ipts, view_pairs="all")
    b = multiview.triangulate_ransac_batch(torch.from_numpy(c["proj"]).to(device), ipts.float(), view_pairs="all")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
