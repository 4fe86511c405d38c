"""Backward kernels vs the reference's autograd (golden gradients) — MI355X only.

Bars: unproject and 2D soft-argmax gradients within 1e-5 max-rel of the reference's f32
autograd (float atomics reorder the sums; forward samples are bit-exact), 3D soft-argmax
gradients within 1e-4 of it; DLT gradients
within 1e-5 of a float64 autograd restatement (oracle/restate_torch.py in float64: torch
svd backward), and within 5e-2 of the f32 reference gradient, whose SVD-backward error is
itself that large for these 2N x 4 systems."""
import numpy as np
import pytest
import torch

from conftest import max_rel
from oracle import restate_torch

pytestmark = pytest.mark.gpu


def _t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


@pytest.mark.parametrize("method", ("sum", "max", "softmax", "conf"))
@pytest.mark.parametrize("ac", (0, 1))
def test_unproject_backward_matches_reference_autograd(golden, device, method, ac):
    from mvn_rocm import op
    d = golden("unproject_small.npz")
    key = f"{method}_ac{ac}"
    feat = _t(d["feat"], device).requires_grad_(True)
    conf = _t(d["conf"], device).requires_grad_(True)
    out = op.unproject_heatmaps(feat, _t(d["proj"], device), _t(d["coords"], device), method,
                                conf if method == "conf" else None, align_corners=bool(ac))
    out.backward(_t(d[f"grad_out_{key}"], device))
    assert max_rel(feat.grad.cpu().numpy(), d[f"grad_feat_{key}"]) <= 1e-5
    if method == "conf":
        assert max_rel(conf.grad.cpu().numpy(), d[f"grad_conf_{key}"]) <= 1e-5


@pytest.mark.parametrize("method", ("sum", "softmax"))
def test_unproject_backward_lds_overflow_path(golden, device, method):
    """Blocks whose footprint exceeds the backward LDS budget scatter with global atomics."""
    from mvn_rocm import op, synth
    vb = synth.volumetric_batch(2, n_views=4, channels=6, heatmap=96, volume=16, seed=3)
    g = torch.randn((2, 6, 16, 16, 16), generator=torch.Generator().manual_seed(1))
    # reference autograd on CPU (the oracle restatement is bit-exact with the reference forward)
    f_cpu = vb.features.clone().requires_grad_(True)
    restate_torch.unproject_heatmaps(f_cpu, vb.proj, vb.coords, method).backward(g)
    f = vb.features.to(device).requires_grad_(True)
    op.unproject_heatmaps(f, vb.proj.to(device), vb.coords.to(device), method).backward(g.to(device))
    assert max_rel(f.grad.cpu().numpy(), f_cpu.grad.numpy()) <= 5e-5     # atomic summation order


@pytest.mark.parametrize("softmax", (True, False))
@pytest.mark.parametrize("mult", (1.0, 1.7))
def test_softargmax_backward_matches_reference_autograd(golden, device, softmax, mult):
    from mvn_rocm import op
    d = golden("softargmax_small.npz")
    key = f"sm{int(softmax)}_m{mult}"
    vol = _t(d["vol"], device).requires_grad_(True)
    xyz, vols = op.integrate_tensor_3d_with_coordinates(vol, _t(d["coords"], device), softmax, multiplier=mult)
    torch.autograd.backward([xyz, vols], [_t(d[f"grad_xyz_{key}"], device), _t(d[f"grad_vol_{key}"], device)])
    assert max_rel(vol.grad.cpu().numpy(), d[f"grad_in_{key}"]) <= 1e-4


def test_softargmax_backward_channel_slice(device):
    """Gradient through the no-copy channel slice used by the bench (strided input)."""
    from mvn_rocm import op, synth
    vb = synth.volumetric_batch(2, channels=1, volume=16, seed=6)
    big = (torch.randn((2, 32, 16, 16, 16), generator=torch.Generator().manual_seed(4)) * 3).to(device)
    big.requires_grad_(True)
    xyz, _ = op.integrate_tensor_3d_with_coordinates(big[:, :17], vb.coords.to(device), multiplier=1.3)
    xyz.sum().backward()
    ref = big.detach().cpu()[:, :17].clone().requires_grad_(True)
    rxyz, _ = restate_torch.integrate_tensor_3d_with_coordinates(ref * 1.3, vb.coords, True)
    rxyz.sum().backward()
    assert max_rel(big.grad[:, :17].cpu().numpy(), ref.grad.numpy()) <= 1e-4
    assert float(big.grad[:, 17:].abs().max()) == 0.0


@pytest.mark.parametrize("case", ("cfg1", "b3n3", "n8"))
@pytest.mark.parametrize("use_conf", (True, False))
def test_dlt_backward(golden, device, case, use_conf):
    from mvn_rocm import multiview
    d = golden("dlt.npz")
    key = f"{case}_c{int(use_conf)}"
    P = d[f"proj_{case}"]
    pts = _t(d[f"points_{case}"], device).requires_grad_(True)
    conf = _t(d[f"conf_{case}"], device).requires_grad_(True) if use_conf else None
    X = multiview.triangulate_batch_of_points(_t(P, device), pts, conf)
    X.backward(_t(d[f"grad_out_{key}"], device))
    # float64 autograd oracle (same algorithm as the reference, solver in f64)
    p64 = torch.from_numpy(d[f"points_{case}"]).double().requires_grad_(True)
    c64 = torch.from_numpy(d[f"conf_{case}"]).double().requires_grad_(True) if use_conf else None
    X64 = restate_torch.triangulate_batch_of_points(torch.from_numpy(P).double(), p64, c64)
    X64.backward(torch.from_numpy(d[f"grad_out_{key}"]).double())
    assert max_rel(pts.grad.cpu().numpy(), p64.grad.numpy()) <= 1e-5
    assert max_rel(pts.grad.cpu().numpy(), d[f"grad_pts_{key}"]) <= 5e-2
    if use_conf:
        assert max_rel(conf.grad.cpu().numpy(), c64.grad.numpy()) <= 1e-5
        assert max_rel(conf.grad.cpu().numpy(), d[f"grad_conf_{key}"]) <= 5e-2


@pytest.mark.parametrize("softmax", (True, False))
@pytest.mark.parametrize("mult", (1.0, 1.7))
def test_softargmax2d_backward_matches_reference_autograd(golden, device, softmax, mult):
    from mvn_rocm import op
    d = golden("softargmax2d.npz")
    key = f"sm{int(softmax)}_m{mult}"
    h = _t(d["hm"], device).requires_grad_(True)
    xy, maps = op.integrate_tensor_2d(h, softmax, multiplier=mult)
    torch.autograd.backward([xy, maps], [_t(d[f"grad_xy_{key}"], device), _t(d[f"grad_maps_{key}"], device)])
    assert max_rel(h.grad.cpu().numpy(), d[f"grad_in_{key}"]) <= 1e-5


@pytest.mark.parametrize("method", ("sum", "softmax", "conf"))
def test_unproject_backward_fixed_point_mode(golden, device, method):
    """The default unprojection backward accumulates in per-call-scaled 64-bit fixed point
    (mvn_unproject_backward_deterministic): two runs are bit-identical — the golden case, a
    config-sized scatter with thousands of colliding taps per pixel, and the LDS-overflow
    (global scatter) path — the gradients stay within 1e-5 of the reference's autograd and
    within 1e-6 of the float-atomic path, also under torch.use_deterministic_algorithms(True)
    (the reference's own training loop runs under autograd.detect_anomaly, train.py:178)."""
    from mvn_rocm import _backward, op, synth
    d = golden("unproject_small.npz")
    key = f"{method}_ac0"

    def run(feat_np, P, coords, conf_np, gout, mode="fixed"):
        prev = _backward.UNPROJECT_BACKWARD
        _backward.UNPROJECT_BACKWARD = mode
        try:
            feat = _t(feat_np, device).requires_grad_(True)
            conf = _t(conf_np, device).requires_grad_(True) if conf_np is not None else None
            out = op.unproject_heatmaps(feat, P, coords, method, conf)
            out.backward(gout)
            return feat.grad.clone(), (conf.grad.clone() if conf is not None else None)
        finally:
            _backward.UNPROJECT_BACKWARD = prev

    P, coords = _t(d["proj"], device), _t(d["coords"], device)
    conf_np = d["conf"] if method == "conf" else None
    g1, c1 = run(d["feat"], P, coords, conf_np, _t(d[f"grad_out_{key}"], device))
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        g2, c2 = run(d["feat"], P, coords, conf_np, _t(d[f"grad_out_{key}"], device), mode="float_atomic")
    finally:
        torch.use_deterministic_algorithms(prev)
    assert torch.equal(g1.view(torch.int32), g2.view(torch.int32))     # the flag forces the fixed path
    assert max_rel(g1.cpu().numpy(), d[f"grad_feat_{key}"]) <= 1e-5
    if method == "conf":
        assert torch.equal(c1.view(torch.int32), c2.view(torch.int32))
        assert max_rel(c1.cpu().numpy(), d[f"grad_conf_{key}"]) <= 1e-5
    for heatmap, volume in ((96, 32), (96, 16)):          # (96, 16): the LDS-overflow global path
        vb = synth.volumetric_batch(2, n_views=4, channels=8, heatmap=heatmap, volume=volume, seed=9)
        cf = np.random.default_rng(9).uniform(0.1, 1, (2, 4, 8)).astype(np.float32) if method == "conf" else None
        gout = torch.randn((2, 8, volume, volume, volume), generator=torch.Generator().manual_seed(2)).to(device)
        a = run(vb.features.numpy(), vb.proj.to(device), vb.coords.to(device), cf, gout)[0]
        b = run(vb.features.numpy(), vb.proj.to(device), vb.coords.to(device), cf, gout)[0]
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        f = run(vb.features.numpy(), vb.proj.to(device), vb.coords.to(device), cf, gout, mode="float_atomic")[0]
        assert max_rel(a.cpu().numpy(), f.cpu().numpy()) <= 1e-6


@pytest.mark.parametrize("scale", (1e-30, 1e-8, 1e8, 1e30))
def test_unproject_backward_fixed_point_scale_follows_the_data(device, scale):
    """The fixed-point exponent is chosen per call from the inputs' magnitudes: gradients
    scaled by 1e-30 ... 1e30 come out as the same relative values (no underflow to zero, no
    overflow) — a fixed 32.32 format would lose the 1e-8 case entirely and overflow at 1e30."""
    from mvn_rocm import op, synth
    vb = synth.volumetric_batch(2, n_views=4, channels=8, heatmap=96, volume=24, seed=12)
    gout = torch.randn((2, 8, 24, 24, 24), generator=torch.Generator().manual_seed(3)).to(device)

    def grad(g):
        f = vb.features.to(device).requires_grad_(True)
        op.unproject_heatmaps(f, vb.proj.to(device), vb.coords.to(device), "softmax").backward(g)
        return f.grad.cpu().numpy().astype(np.float64)

    base = grad(gout)
    scaled = grad(gout * scale) / scale
    assert np.abs(base).max() > 0
    assert max_rel(scaled, base) <= 1e-6


def _grads(device, method, feat, P, coords, conf, gout, mode):
    """(grad_feat, grad_conf) of mvn_rocm's unprojection with backward `mode`, as numpy."""
    from mvn_rocm import _backward, op
    prev = _backward.UNPROJECT_BACKWARD
    _backward.UNPROJECT_BACKWARD = mode
    try:
        f = feat.to(device).requires_grad_(True)
        c = conf.to(device).requires_grad_(True) if conf is not None else None
        op.unproject_heatmaps(f, P.to(device), coords.to(device), method, c).backward(gout.to(device))
        return f.grad.cpu().numpy(), (c.grad.cpu().numpy() if c is not None else None)
    finally:
        _backward.UNPROJECT_BACKWARD = prev


def _ref_grads(method, feat, P, coords, conf, gout, dtype=torch.float32):
    """The reference's autograd (ATen grid_sampler / softmax / einsum backward) through the
    op-for-op restatement of op.py:99-163, on the CPU."""
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)       # the restatement's own buffers (op.py:104, 111) follow it
    try:
        f = feat.to(dtype).clone().requires_grad_(True)
        c = conf.to(dtype).clone().requires_grad_(True) if conf is not None else None
        restate_torch.unproject_heatmaps(f, P.to(dtype), coords.to(dtype), method, c).backward(gout.to(dtype))
        return f.grad.numpy(), (c.grad.numpy() if c is not None else None)
    finally:
        torch.set_default_dtype(prev)


def _same_nonfinite(a, b):
    """NaN / +inf / -inf at exactly the same elements."""
    assert np.array_equal(np.isnan(a), np.isnan(b))
    assert np.array_equal(np.isposinf(a), np.isposinf(b))
    assert np.array_equal(np.isneginf(a), np.isneginf(b))


@pytest.mark.parametrize("mode", ("fixed", "float_atomic"))
@pytest.mark.parametrize("method", ("sum", "max", "softmax", "conf"))
@pytest.mark.parametrize("what", ("grad_nan", "feat_nan", "feat_inf", "conf_inf"))
def test_unproject_backward_nonfinite_follow_the_reference(device, mode, method, what):
    """Non-finite inputs reach exactly the gradient elements they reach in the reference's
    autograd (ATen grid_sampler backward confines a NaN upstream gradient to the taps of its
    voxel, a zero tap weight included; 'sum' / 'conf' feature gradients do not read the
    features, so a NaN feature leaves them finite; 'max' routes the gradient to the NaN view;
    softmax spreads it over the voxel's views): the NaN / +inf / -inf pattern is compared
    element by element, and the finite elements within 1e-5 of the reference."""
    from mvn_rocm import synth
    if what == "conf_inf" and method != "conf":
        pytest.skip("confidences only enter conf*")
    vb = synth.volumetric_batch(2, n_views=4, channels=4, heatmap=32, volume=16, seed=21)
    feat, P, coords = vb.features.clone(), vb.proj, vb.coords
    conf = torch.from_numpy(np.random.default_rng(21).uniform(0.2, 1.0, (2, 4, 4)).astype(np.float32)) \
        if method == "conf" else None
    gout = torch.randn((2, 4, 16, 16, 16), generator=torch.Generator().manual_seed(5))
    if what == "grad_nan":
        gout[0, 1, 8, 8, 8] = float("nan")
        gout[1, 2, 3, 9, 5] = float("nan")
    elif what == "feat_nan":
        feat[0, 1, 2, 16, 16] = float("nan")       # inside every view's footprint at this geometry
        feat[1, 3, 0, 15, 17] = float("nan")
    elif what == "feat_inf":
        feat[0, 2, 1, 16, 15] = float("inf")
        feat[1, 0, 3, 17, 16] = -float("inf")
    else:
        conf[0, 1, 2] = float("inf")
    ours, ours_c = _grads(device, method, feat, P, coords, conf, gout, mode)
    ref, ref_c = _ref_grads(method, feat, P, coords, conf, gout)
    _same_nonfinite(ours, ref)
    fin = np.isfinite(ref)
    assert fin.any()
    assert max_rel(ours[fin], ref[fin]) <= 1e-5
    if method == "conf":
        _same_nonfinite(ours_c, ref_c)
        cf = np.isfinite(ref_c)
        if cf.any():
            assert max_rel(ours_c[cf], ref_c[cf]) <= 1e-5
    if what in ("feat_nan", "feat_inf") and method in ("sum", "conf"):
        assert np.isfinite(ours).all()               # the feature gradient does not read feat


@pytest.mark.parametrize("mode", ("fixed", "float_atomic"))
@pytest.mark.parametrize("method", ("softmax", "conf"))
@pytest.mark.parametrize("what", ("feat_inf", "conf_inf"))
def test_unproject_backward_direct_path_partial_tiles_nonfinite(device, mode, method, what):
    """The global-atomic path (footprints past the LDS budget: 96^2 maps on a coarse 13^3 grid)
    on partial tiles (13 is no multiple of the tile): threads past the volume's edge scatter
    nothing, so an infinite confidence or feature produces +-inf exactly where the reference's
    autograd does and no NaN at voxel 0's taps."""
    from mvn_rocm import synth
    if what == "conf_inf" and method != "conf":
        pytest.skip("confidences only enter conf*")
    vb = synth.volumetric_batch(2, n_views=4, channels=4, heatmap=96, volume=13, seed=8)
    feat, P, coords = vb.features.clone(), vb.proj, vb.coords
    conf = torch.from_numpy(np.random.default_rng(8).uniform(0.2, 1.0, (2, 4, 4)).astype(np.float32)) \
        if method == "conf" else None
    gout = torch.randn((2, 4, 13, 13, 13), generator=torch.Generator().manual_seed(9))
    # the path under test: every 4x8x8 tile's footprints (pitch x rows, summed over the views)
    # exceed the backward's 1,022 LDS slots (unproject_bwd.hip kZero), so no tile stages
    from test_gpu_parity import tile_footprints
    assert (tile_footprints(P.numpy(), coords.numpy(), 96, 96, (4, 8, 8)).sum(1) > 1022).all()
    if what == "feat_inf":
        feat[0, 2, 1, 48, 47] = float("inf")
        feat[1, 0, 3, 47, 48] = -float("inf")
    else:
        conf[0, 1, 2] = float("inf")
    ours, ours_c = _grads(device, method, feat, P, coords, conf, gout, mode)
    ref, ref_c = _ref_grads(method, feat, P, coords, conf, gout)
    assert not (np.isfinite(ref).all() and (ref_c is None or np.isfinite(ref_c).all()))   # the input reached
    _same_nonfinite(ours, ref)
    fin = np.isfinite(ref)
    assert fin.any()
    assert max_rel(ours[fin], ref[fin]) <= 5e-5          # atomic summation order
    if method == "conf":
        _same_nonfinite(ours_c, ref_c)


def test_unproject_backward_fixed_point_keeps_every_element_exact(golden, device):
    """Per-element parity of the default (fixed-point) backward with the reference's own
    autograd in one call whose gradients span 1e-12 ... 1e8: frame 1's upstream gradient is
    1e8 x frame 0's, and channel 2 of frame 0 is another 1e-12 below.  The reference gradient
    is the golden captured from mvn/utils/op.py's autograd in the build container
    (tests/golden/unproject_bwd_elementwise.npz), not recomputed here: ATen's CPU
    grid_sampler backward is host-dependent — on this box's EPYC it recomputes the sampling
    coordinate with a different rounding than its forward and differs from the container's
    Xeon result by up to 9.3e-4 element-wise (profiles/r20_bwd_host_probe_epyc.txt), while the
    Xeon result is the exact sum of the forward's own tap products to 2.9e-7.
      'sum' (non-negative upstream gradient): EVERY nonzero element within 1e-5 relative of the
        reference, zeros at exactly the reference's zeros; the float-atomic path (same
        products, float sums) agrees with the fixed-point one within 1e-6 per element.
      'softmax' (sharpened features, both signs; coefficients spanning e^-20): per frame
        within 5e-5 of the reference (its own f32 gradient is 1.6e-5 / 2.3e-5 from its float64
        re-run)."""
    d = golden("unproject_bwd_elementwise.npz")
    feat, P, coords = (torch.from_numpy(d[k]) for k in ("feat", "proj", "coords"))
    gout = torch.from_numpy(d["grad_out_sum"])
    ref = d["grad_feat_sum"]
    ours = _grads(device, "sum", feat, P, coords, None, gout, "fixed")[0]
    flt = _grads(device, "sum", feat, P, coords, None, gout, "float_atomic")[0]
    assert np.array_equal(ours == 0, ref == 0) and np.array_equal(flt == 0, ref == 0)
    nz = ref != 0
    rel = np.abs(ours[nz].astype(np.float64) - ref[nz]) / np.abs(ref[nz].astype(np.float64))
    assert rel.max() <= 1e-5, rel.max()
    rel_f = np.abs(ours[nz].astype(np.float64) - flt[nz]) / np.abs(flt[nz].astype(np.float64))
    assert rel_f.max() <= 1e-6, rel_f.max()
    # the two frames and the tiny channel each really are at their own scale
    assert np.abs(ref[1]).max() > 1e6 * np.abs(ref[0]).max() > 0
    assert 0 < np.abs(ref[0, :, 2]).max() < 1e-10 * np.abs(ref[0]).max()

    ours = _grads(device, "softmax", feat * 20.0, P, coords, None, torch.from_numpy(d["grad_out_softmax"]), "fixed")[0]
    ref = d["grad_feat_softmax"]
    for b in range(2):
        assert np.abs(ref[b]).max() > 0
        assert max_rel(ours[b], ref[b]) <= 5e-5
