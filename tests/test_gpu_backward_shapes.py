"""The backward kernels at the shapes, view counts and dtypes a training run uses — MI355X only.

tests/test_gpu_backward.py checks the numerics in depth at 4 views, f32 and small volumes;
here the same kernels (csrc/unproject_bwd.hip, csrc/backward.hip) run where their code takes
other paths: the 8-view instantiation and partial view counts of the unprojection backward on
the LDS and the direct-global path, its bf16 instantiations, the soft-argmax backward past its
grid-stride and partial-fold thresholds with J % 4 != 0 and bf16, -inf logits, the DLT
backward over several blocks, and the whole training step against the float64 reference chain.

Every reference is autograd through oracle/restate_torch.py on the CPU (oracle/backward_cases.py
builds the inputs and the references; tests/test_backward_refs.py pins their own error).  The
metric is max |ours - ref| / max |ref| PER view, joint or frame (backward_cases.max_rel_per):
under the real loss one cross-entropy voxel per joint dominates a global maximum.  Bars: the
project's own (1e-5 unprojection on the LDS path, 5e-5 on the global-atomic path, 1e-4
soft-argmax and training step, 1e-5 DLT); a bf16 result r = rn_bf16(ref + d), |d| <= tol *
max|ref|, is held to |r - ref| <= 2^-8 |ref| + 1.01 tol max|ref| element by element."""
import functools

import numpy as np
import pytest
import torch

from oracle import backward_cases as cases
from oracle import restate_torch
from oracle.backward_cases import bf16_round, max_rel_per
from test_gpu_backward import _grads, _ref_grads, _same_nonfinite
from test_gpu_parity import tile_footprints

pytestmark = pytest.mark.gpu

BF16_HALF_ULP = 2.0 ** -8


def _views_first(a):
    return np.moveaxis(a, 1, 0)


def _assert_bf16_bound(ours, ref, tol, keep_dims, what=""):
    """ours = rn_bf16(ref + d) with |d| <= tol * max|ref| (max over the trailing dimensions of
    each of the first `keep_dims`): |ours - ref| <= 2^-8 |ref| + 1.01 tol max|ref|, per element.
    Prints the worst element as a fraction of its bound."""
    ours, ref = np.asarray(ours, np.float64), np.asarray(ref, np.float64)
    lead = ref.shape[:keep_dims]
    o2, r2 = ours.reshape(int(np.prod(lead)), -1), ref.reshape(int(np.prod(lead)), -1)
    den = np.abs(r2).max(1, keepdims=True)
    assert (den > 0).all()
    bound = BF16_HALF_ULP * np.abs(r2) + 1.01 * tol * den
    frac = (np.abs(o2 - r2) / bound).max()
    print(f"{what} bf16 worst element / bound: {frac:.3f}")
    assert frac <= 1.0, frac


# ---------------------------------------------------------------- 1. unprojection: view counts
@functools.lru_cache(maxsize=None)
def _unproject_case(path, n_views):
    c = cases.unproject_case(path, n_views)
    hm = c["heatmap"]
    sums = tile_footprints(c["proj"].numpy(), c["coords"].numpy(), hm, hm, cases.TILE).sum(1)
    return c, sums


@functools.lru_cache(maxsize=None)
def _unproject_ref(path, n_views, method):
    c, _ = _unproject_case(path, n_views)
    return _ref_grads(method, c["feat"], c["proj"], c["coords"], c["conf"] if method == "conf" else None, c["gout"])


@pytest.mark.parametrize("path", ("lds", "direct"))
@pytest.mark.parametrize("mode", ("fixed", "float_atomic"))
@pytest.mark.parametrize("method", ("sum", "max", "softmax", "conf"))
@pytest.mark.parametrize("n_views", cases.VIEW_COUNTS)
def test_unproject_backward_view_counts(device, n_views, method, mode, path):
    """1-3 views run the 4-view instantiation with dead unrolled views (its v < N guards),
    5-8 the 8-view instantiation (own LDS layout, eight footprints against the same 1,022
    slots), each on the LDS path (partial tiles on every axis, a partial channel group) and on
    the direct global-atomic path, in both accumulation modes.  Per VIEW within 1e-5 (LDS) /
    5e-5 (direct: atomic summation order) of the reference's f32 autograd; 8 views in
    fixed-point mode bit-identical across two runs."""
    c, sums = _unproject_case(path, n_views)
    if path == "lds":
        assert sums.max() <= cases.LDS_SLOTS - 64           # margin: the kernel rounds in f32
        bar = 1e-5
    else:
        over = sums > cases.LDS_SLOTS + 64
        assert over.all() if n_views >= 3 else over.any()
        bar = 5e-5
    conf = c["conf"] if method == "conf" else None
    ours, ours_c = _grads(device, method, c["feat"], c["proj"], c["coords"], conf, c["gout"], mode)
    ref, ref_c = _unproject_ref(path, n_views, method)
    per_view = max_rel_per(_views_first(ours), _views_first(ref), 1)
    print(f"grad_feat per view: {per_view.max():.2e}")
    assert np.abs(_views_first(ref)).reshape(n_views, -1).max(1).min() > 0
    assert per_view.max() <= bar, per_view
    if method == "conf":
        per_view_c = max_rel_per(_views_first(ours_c), _views_first(ref_c), 1)
        print(f"grad_conf per view: {per_view_c.max():.2e}")
        assert per_view_c.max() <= bar, per_view_c
    if mode == "fixed" and n_views == 8:
        again, again_c = _grads(device, method, c["feat"], c["proj"], c["coords"], conf, c["gout"], mode)
        assert np.array_equal(ours.view(np.uint32), again.view(np.uint32))
        if method == "conf":
            assert np.array_equal(ours_c.view(np.uint32), again_c.view(np.uint32))


@pytest.mark.parametrize("mode", ("fixed", "float_atomic"))
def test_unproject_backward_rejects_more_than_8_views(device, mode):
    """The forward takes any view count; the backward kernels are instantiated for up to 8:
    a 9-view backward raises (MVN_ERR_SHAPE), it never returns a silent zero gradient."""
    from mvn_rocm import _backward, _lib, op, synth
    vb = synth.volumetric_batch(1, n_views=9, channels=2, heatmap=20, volume=8, seed=2)
    feat = vb.features.to(device).requires_grad_(True)
    out = op.unproject_heatmaps(feat, vb.proj.to(device), vb.coords.to(device), "sum")
    assert torch.isfinite(out).all()
    prev = _backward.UNPROJECT_BACKWARD
    _backward.UNPROJECT_BACKWARD = mode
    try:
        with pytest.raises(_lib.MvnError):
            out.sum().backward()
    finally:
        _backward.UNPROJECT_BACKWARD = prev
    assert feat.grad is None


# ---------------------------------------------------------------- 2. unprojection: bf16
def _grads_dtypes(device, method, feat, P, coords, conf, gout, mode, out_dtype):
    """(grad_feat, grad_conf) as torch CPU tensors in the dtypes the op returns.  The forward
    has no f32-features -> bf16-volume instantiation and autograd casts an upstream gradient to
    its output's dtype, so that combination reaches the backward only through the custom op
    (torch.ops.mvn_rocm.unproject_backward) itself: it is called directly."""
    from mvn_rocm import _backward, _ops, op
    prev = _backward.UNPROJECT_BACKWARD
    _backward.UNPROJECT_BACKWARD = mode
    try:
        if feat.dtype == torch.float32 and out_dtype == torch.bfloat16:
            assert gout.dtype == torch.bfloat16
            gf, gc = _ops.call(_backward.unproject_bwd, feat.to(device), P.to(device), coords.to(device),
                               conf.to(device) if conf is not None else None, gout.to(device),
                               op.aggregation_code(method), False, conf is not None)
            return gf.cpu(), (gc.cpu() if conf is not None else None)
        f = feat.to(device).requires_grad_(True)
        c = conf.to(device).requires_grad_(True) if conf is not None else None
        out = op.unproject_heatmaps(f, P.to(device), coords.to(device), method, c, out_dtype=out_dtype)
        assert out.dtype == out_dtype and gout.dtype == out_dtype
        out.backward(gout.to(device))
        return f.grad.cpu(), (c.grad.cpu() if c is not None else None)
    finally:
        _backward.UNPROJECT_BACKWARD = prev


_BF16_COMBOS = {"bf16feat_f32grad": (torch.bfloat16, torch.float32),
                "f32feat_bf16grad": (torch.float32, torch.bfloat16),
                "bf16feat_bf16grad": (torch.bfloat16, torch.bfloat16)}


def _unproject_bf16(device, n_views, method, combo, mode):
    feat_dt, grad_dt = _BF16_COMBOS[combo]
    c, sums = _unproject_case("lds", n_views)
    assert sums.max() <= cases.LDS_SLOTS - 64
    feat, gout = c["feat"].to(feat_dt), c["gout"].to(grad_dt)
    conf = c["conf"] if method == "conf" else None
    ours, ours_c = _grads_dtypes(device, method, feat, c["proj"], c["coords"], conf, gout, mode, grad_dt)
    # the reference on the rounded inputs, computed in f32
    ref, ref_c = _ref_grads(method, feat.float(), c["proj"], c["coords"], conf, gout.float())
    assert ours.dtype == feat_dt
    if feat_dt == torch.float32:
        per_view = max_rel_per(_views_first(ours.numpy()), _views_first(ref), 1)
        print(f"{combo} grad_feat per view: {per_view.max():.2e}")
        assert per_view.max() <= 1e-5, per_view
    else:
        _assert_bf16_bound(_views_first(ours.float().numpy()), _views_first(ref), 1e-5, 1, f"{combo} grad_feat")
    if method == "conf":
        assert ours_c.dtype == torch.float32
        per_view_c = max_rel_per(_views_first(ours_c.numpy()), _views_first(ref_c), 1)
        print(f"{combo} grad_conf per view: {per_view_c.max():.2e}")
        assert per_view_c.max() <= 1e-5, per_view_c


@pytest.mark.parametrize("n_views", (4, 8))
@pytest.mark.parametrize("combo", tuple(_BF16_COMBOS))
@pytest.mark.parametrize("method", ("sum", "softmax", "conf"))
def test_unproject_backward_bf16(device, method, combo, n_views):
    """The three (feature, grad_out) dtype instantiations no other test runs, of the backward
    kernel and of fix_scale_planes, at 4 and 8 views in fixed-point mode.  grad_conf is f32 (the
    f32 bar), grad_feat follows the features: f32 at the f32 bar, bf16 at the derived bound.
    (f32 features with a bf16 grad_out go through the custom op directly, see _grads_dtypes.)
    Measured: f32 results 1.4e-6 ... 2.7e-6 per view; the worst bf16 element at 0.96 ... 0.98 of
    its bound — the bound is the half-ulp of bf16 plus 1% of the f32 bar, so a correctly rounded
    result comes that close by construction."""
    _unproject_bf16(device, n_views, method, combo, "fixed")


@pytest.mark.parametrize("combo", tuple(_BF16_COMBOS))
def test_unproject_backward_bf16_float_atomic(device, combo):
    _unproject_bf16(device, 8, "conf", combo, "float_atomic")


# ---------------------------------------------------------------- 3. soft-argmax: large volumes
@functools.lru_cache(maxsize=None)
def _sa_case():
    return cases.softargmax_case()


def _sa_ours(device, logits, coords, softmax, mult, grad_xyz, idx, mix, return_volumes=True):
    from mvn_rocm import op
    v = logits.to(device).requires_grad_(True)
    xyz, vols = op.integrate_tensor_3d_with_coordinates(v, coords.to(device), softmax, multiplier=mult,
                                                        return_volumes=return_volumes)
    if not return_volumes:
        assert vols is None and mix == "xyz"
    cases.softargmax_loss(xyz, vols, grad_xyz.to(device), idx, mix).backward()
    return v.grad


@pytest.mark.parametrize("mix", ("full", "xyz", "vol"))
@pytest.mark.parametrize("mult", (1.0, 1.7))
@pytest.mark.parametrize("softmax", (True, False))
def test_softargmax_backward_large_odd_volume(device, softmax, mult, mix):
    """(33, 63, 65) = 135,135 voxels, 5 joints: 66 pass-1 partials (the 64-lane fold takes a
    second trip), more voxels than the apply kernel's 64 x 256 threads (grid stride), an odd
    size (partial last strides), a second joint group with one live wave.  Upstream gradients
    shaped like training: a small grad_xyz and one cross-entropy voxel per joint.  Per JOINT
    within 1e-4 of float64 autograd (the f32 reference itself: <= 2.6e-5)."""
    c = _sa_case()
    ours = _sa_ours(device, c["logits"], c["coords"], softmax, mult, c["grad_xyz"], c["idx"], mix)
    ref = cases.softargmax_ref_grad(c["logits"], c["coords"], softmax, mult, c["grad_xyz"], c["idx"], mix)
    per_joint = max_rel_per(ours.cpu().numpy(), ref, 2)
    print(f"softmax={softmax} mult={mult} {mix}: per joint {per_joint.max():.2e}")
    assert np.isfinite(ours.cpu().numpy()).all()
    if softmax or mix != "vol":            # relu + a cross-entropy voxel at a non-positive logit: all zero
        assert np.abs(ref).reshape(10, -1).max(1).min() > 0
    assert per_joint.max() <= 1e-4, per_joint


@pytest.mark.parametrize("softmax", (True, False))
def test_softargmax_backward_without_returned_volumes(device, softmax):
    """return_volumes=False: the xyz-only gradient, bit for bit that of the returning call."""
    c = _sa_case()
    args = (device, c["logits"], c["coords"], softmax, 1.7, c["grad_xyz"], c["idx"], "xyz")
    a = _sa_ours(*args, return_volumes=True)
    b = _sa_ours(*args, return_volumes=False)
    assert float(a.abs().max()) > 0
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_softargmax_backward_large_strided_input(device):
    """big[:, :5] of a (2, 8, ...) tensor (batch / joint strides, no copy) under the full loss:
    the slice's gradient within 1e-4 per joint, the rest of big exactly 0."""
    from mvn_rocm import op
    c = cases.softargmax_case(channels=8)
    big = c["logits"].to(device).requires_grad_(True)
    xyz, vols = op.integrate_tensor_3d_with_coordinates(big[:, :5], c["coords"].to(device), multiplier=1.7)
    cases.softargmax_loss(xyz, vols, c["grad_xyz"].to(device), c["idx"], "full").backward()
    ref = cases.softargmax_ref_grad(c["logits"][:, :5], c["coords"], True, 1.7, c["grad_xyz"], c["idx"], "full")
    per_joint = max_rel_per(big.grad[:, :5].cpu().numpy(), ref, 2)
    print(f"strided: per joint {per_joint.max():.2e}")
    assert per_joint.max() <= 1e-4, per_joint
    assert float(big.grad[:, 5:].abs().max()) == 0.0


@pytest.mark.parametrize("softmax", (True, False))
@pytest.mark.parametrize("vol_dt,out_dt", ((torch.float32, torch.bfloat16), (torch.bfloat16, torch.float32),
                                           (torch.bfloat16, torch.bfloat16)))
def test_softargmax_backward_bf16_large_volume(device, vol_dt, out_dt, softmax):
    """The three (volume, grad_vol, grad_in) instantiations no other test runs, at the large
    odd shape, multiplier 1.7.  The reference is float64 autograd on the bf16-rounded logits
    with the same (bf16-rounded where the returned volume is bf16) upstream gradients: a small
    grad_xyz and the cross-entropy gradient -1 / (p + 1e-6) / (B J) at one voxel per joint, p
    the reference's.  f32 grad_in: 1e-4 per joint; bf16 grad_in: the derived bound."""
    from mvn_rocm import _backward, _ops, op
    c = _sa_case()
    logits = c["logits"].to(vol_dt)
    with torch.no_grad():
        _, p = restate_torch.integrate_tensor_3d_with_coordinates(logits.double() * 1.7, c["coords"].double(), softmax)
    gv = cases.ce_grad_vol(p, c["idx"]).to(out_dt)
    if vol_dt == torch.float32:
        # the forward returns an f32 volume's normalised volume in f32 only, and autograd casts
        # an upstream gradient to that dtype: a bf16 grad_vol reaches the kernel only through
        # the custom op (torch.ops.mvn_rocm.softargmax3d_backward) itself
        grad_in = _ops.call(_backward.softargmax3d_bwd, logits.to(device), c["coords"].to(device), softmax, 1.7,
                            c["grad_xyz"].to(device), gv.to(device))
    else:
        v = logits.to(device).requires_grad_(True)
        xyz, vols = op.integrate_tensor_3d_with_coordinates(v, c["coords"].to(device), softmax, multiplier=1.7,
                                                            out_dtype=out_dt)
        assert vols.dtype == out_dt and xyz.dtype == torch.float32
        torch.autograd.backward([xyz, vols], [c["grad_xyz"].to(device), gv.to(device)])
        grad_in = v.grad
    assert grad_in.dtype == vol_dt
    _, _, ref = cases.softargmax_ref_explicit(logits, c["coords"], softmax, 1.7, c["grad_xyz"], gv)
    ours = grad_in.float().cpu().numpy()
    assert np.isfinite(ours).all()
    if vol_dt == torch.float32:
        per_joint = max_rel_per(ours, ref, 2)
        print(f"f32 volume, bf16 grad_vol, softmax={softmax}: per joint {per_joint.max():.2e}")
        assert per_joint.max() <= 1e-4, per_joint
    else:
        _assert_bf16_bound(ours, ref, 1e-4, 2, f"bf16 volume, {out_dt} grad_vol, softmax={softmax}: grad_in")


# ---------------------------------------------------------------- 4. -inf logits
@pytest.mark.parametrize("softmax", (True, False))
@pytest.mark.parametrize("dt", (torch.float32, torch.bfloat16))
def test_softargmax_neg_inf_logits_follow_torch(device, dt, softmax):
    """A masked (-inf) logit has probability 0: torch's softmax / einsum and their autograd give
    finite joints and volumes and a gradient that is exactly 0 at the masked voxels.  Joint 0
    is clean; joint 1 has -inf at voxels 0-63 (every lane's FIRST element of the backward's
    pass 1) and over the whole second 2,048-voxel chunk; joint 2 has a single -inf; joint 3 is
    -inf everywhere, where torch returns NaN (softmax) — and so do we."""
    from mvn_rocm import op, synth
    g = torch.Generator().manual_seed(44)
    coords = synth.volumetric_batch(1, channels=1, volume=16, seed=4).coords
    clean = (3.0 * torch.randn((1, 4, 4096), generator=g)).to(dt)
    vol = clean.clone()
    vol[0, 1, :64] = -float("inf")
    vol[0, 1, 2048:] = -float("inf")
    vol[0, 2, 3000] = -float("inf")
    vol[0, 3, :] = -float("inf")
    masked = torch.isinf(vol).view(1, 4, 16, 16, 16).numpy()
    gx = 1e-3 * torch.randn((1, 4, 3), generator=g)
    gv = (0.1 * torch.randn((1, 4, 16, 16, 16), generator=g)).to(dt)
    mult = 1.7

    def ours_of(x):
        v = x.view(1, 4, 16, 16, 16).to(device).requires_grad_(True)
        xyz, vols = op.integrate_tensor_3d_with_coordinates(v, coords.to(device), softmax, multiplier=mult)
        torch.autograd.backward([xyz, vols], [gx.to(device), gv.to(device)])
        return xyz.detach().cpu().numpy(), vols.detach().float().cpu().numpy(), v.grad.cpu()

    xyz, vols, grad_t = ours_of(vol)
    assert grad_t.dtype == dt
    grad = grad_t.float().numpy()
    rxyz, rvols, rgrad = cases.softargmax_ref_explicit(vol.float().view(1, 4, 16, 16, 16), coords, softmax, mult, gx,
                                                       gv.float())
    live = slice(0, 3) if softmax else slice(0, 4)          # relu(-inf) = 0: joint 3 is finite too
    assert np.isfinite(rxyz[:, live]).all() and np.isfinite(rgrad[:, live]).all()
    # forward: finite, and the reference's values
    assert np.isfinite(xyz[:, live]).all() and np.isfinite(vols[:, live]).all()
    assert (vols[masked] == 0).all() if not softmax else (vols[:, live][masked[:, live]] == 0).all()
    if dt == torch.float32:
        assert np.abs(xyz[:, live] - rxyz[:, live]).max() <= 1e-5 * np.abs(rxyz[:, live]).max()
    # backward: finite, exactly 0 at the masked voxels, per joint within the bar elsewhere
    assert np.isfinite(grad[:, live]).all()
    assert (rgrad[:, live][masked[:, live]] == 0).all()
    assert (grad[:, live][masked[:, live]] == 0).all()
    if dt == torch.float32:
        per_joint = max_rel_per(grad[:, :3], rgrad[:, :3], 2)
        print(f"-inf, softmax={softmax}: per joint {per_joint.max():.2e}")
        assert per_joint.max() <= 1e-4, per_joint
    else:
        _assert_bf16_bound(grad[:, :3], rgrad[:, :3], 1e-4, 2, f"-inf, softmax={softmax}: grad_in")
    # joint 0 does not see the other joints' masks
    grad_clean = ours_of(clean)[2].float().numpy()
    assert np.array_equal(grad[0, 0].view(np.uint32), grad_clean[0, 0].view(np.uint32))
    # a joint that is -inf everywhere: torch's NaN (softmax), zeros (relu)
    if softmax:
        assert np.isnan(rgrad[0, 3]).all() and np.isnan(rxyz[0, 3]).all()
        assert np.isnan(grad[0, 3]).all() and np.isnan(xyz[0, 3]).all()
    else:
        assert (rgrad[0, 3] == 0).all() and (grad[0, 3] == 0).all()
    _same_nonfinite(grad, rgrad)


def test_softargmax_relu_nan_voxel_follows_torch(device):
    """relu mode, one NaN voxel in joint 1: torch's relu keeps the NaN (the joint's coordinates
    are NaN, the returned volume holds it at that voxel) and its backward masks with x <= 0, so
    the NaN voxel receives mult * d like a positive one and every gradient stays finite."""
    from mvn_rocm import op, synth
    g = torch.Generator().manual_seed(45)
    coords = synth.volumetric_batch(1, channels=1, volume=16, seed=4).coords
    vol = 3.0 * torch.randn((1, 3, 4096), generator=g)
    vol[0, 1, 1500] = float("nan")
    gx = 1e-3 * torch.randn((1, 3, 3), generator=g)
    gv = 0.1 * torch.randn((1, 3, 16, 16, 16), generator=g)
    mult = 1.7
    v = vol.view(1, 3, 16, 16, 16).to(device).requires_grad_(True)
    xyz, vols = op.integrate_tensor_3d_with_coordinates(v, coords.to(device), False, multiplier=mult)
    torch.autograd.backward([xyz, vols], [gx.to(device), gv.to(device)])
    xyz, vols, grad = xyz.detach().cpu().numpy(), vols.detach().cpu().numpy(), v.grad.cpu().numpy()
    rxyz, rvols, rgrad = cases.softargmax_ref_explicit(vol.view(1, 3, 16, 16, 16), coords, False, mult, gx, gv)
    assert np.isnan(rxyz[0, 1]).all() and np.isfinite(rxyz[0, (0, 2), :]).all()
    assert np.isnan(rvols).sum() == 1 and np.isfinite(rgrad).all()
    assert rgrad.reshape(1, 3, -1)[0, 1, 1500] != 0
    _same_nonfinite(xyz, rxyz)
    _same_nonfinite(vols, rvols)
    _same_nonfinite(grad, rgrad)
    per_joint = max_rel_per(grad, rgrad, 2)
    print(f"relu, NaN voxel: per joint {per_joint.max():.2e}")
    assert per_joint.max() <= 1e-4, per_joint


# ---------------------------------------------------------------- 5. DLT: several blocks
def _joints_first(a):
    return np.moveaxis(a, 2, 1)          # (B, N, J, ..) -> (B, J, N, ..)


@functools.lru_cache(maxsize=None)
def _dlt_refs(n_views, use_conf):
    c = cases.dlt_case(n_views)
    conf = c["conf"] if use_conf else None
    _, gp1, gc1 = restate_torch.triangulate_batch_of_points_f32_design(c["proj"], c["points"], conf, c["gout"])
    gp2, _ = cases.dlt_ref_f64(c["proj"], c["points"], conf, c["gout"])
    return c, gp1.numpy(), gc1.numpy(), gp2


@pytest.mark.parametrize("use_conf", (True, False))
@pytest.mark.parametrize("n_views", (2, 3, 4, 8))
def test_dlt_backward_multi_block(device, n_views, use_conf):
    """8 frames x 17 joints = 136 threads: three 64-thread blocks, the last with 8 live threads
    (the goldens stay inside one block), at 2-8 views, with zero-confidence views (4 and 8
    views: the Givens fold skips their zero rows).

    Reference 1 forms the design matrix in f32 like the kernel and the reference's
    multiview.py:150-152, then solves and back-propagates in float64
    (restate_torch.triangulate_batch_of_points_f32_design): grad_pts and grad_conf within 1e-5
    per JOINT (max over the joint's views).  Reference 2 is the pure-float64 restatement:
    grad_pts within 1e-5 per joint; no assertion on grad_conf against it — the f32 rounding of
    A alone moves grad_conf by 4e-6 ... 6e-6 per frame at 3-8 views and 2e-4 at 2 views
    (tests/test_backward_refs.py), which is a property of the f32 design matrix both we and
    the reference share, not of the solver.  Zero-confidence views: grad_pts exactly 0,
    grad_conf finite and reference 1's.  A gradient requested for the points alone or the
    confidences alone is bit for bit that half of the run requesting both."""
    from mvn_rocm import multiview
    c, gp1, gc1, gp2 = _dlt_refs(n_views, use_conf)
    P, gout = c["proj"].to(device), c["gout"].to(device)

    def run(want_pts, want_conf):
        pts = c["points"].to(device).requires_grad_(want_pts)
        conf = c["conf"].to(device).requires_grad_(want_conf) if use_conf else None
        multiview.triangulate_batch_of_points(P, pts, conf).backward(gout)
        return (pts.grad.cpu().numpy() if want_pts else None,
                conf.grad.cpu().numpy() if (use_conf and want_conf) else None)

    gp, gc = run(True, use_conf)
    assert gp.shape == (8, n_views, 17, 2) and np.isfinite(gp).all()
    e1 = max_rel_per(_joints_first(gp), _joints_first(gp1), 2)
    e2 = max_rel_per(_joints_first(gp), _joints_first(gp2), 2)
    print(f"n_views={n_views} conf={use_conf}: grad_pts per joint {e1.max():.2e} (f32 design), {e2.max():.2e} (f64)")
    assert e1.max() <= 1e-5, e1
    assert e2.max() <= 1e-5, e2
    if use_conf:
        assert np.isfinite(gc).all()
        ec = max_rel_per(_joints_first(gc), _joints_first(gc1), 2)
        print(f"n_views={n_views}: grad_conf per joint {ec.max():.2e} (f32 design)")
        assert ec.max() <= 1e-5, ec
        zero = (c["conf"] == 0).numpy()
        assert zero.any() == (n_views >= 4)
        assert (gp[zero] == 0).all()
        only_p, none_c = run(True, False)
        none_p, only_c = run(False, True)
        assert none_c is None and none_p is None
        assert np.array_equal(only_p.view(np.uint32), gp.view(np.uint32))
        assert np.array_equal(only_c.view(np.uint32), gc.view(np.uint32))


# ---------------------------------------------------------------- 7. the training step
@pytest.mark.parametrize("coords_kind", ("volume", "cuboids"))
@pytest.mark.parametrize("scale", (1.0, 10.0))
def test_training_step_gradient_matches_float64_reference(device, scale, coords_kind):
    """Unprojection (softmax) -> channel slice [:5] -> soft-argmax -> L1 + 0.01 *
    VolumetricCELoss -> backward(), against the same chain through restate_torch in float64
    (restate_torch.volumetric_ce_loss included): the loss within 1e-5, grad_feat within 1e-4
    per FRAME, the unused channels' gradient exactly 0.  (The f32 reference chain is 3e-6 /
    1e-5 per frame from float64 at scale 1 / 10.)  'cuboids' runs both ops on in-kernel
    coordinates; its reference takes the numpy restatement of the same coordinate volume."""
    from mvn_rocm import loss as mloss
    from mvn_rocm import op
    if coords_kind == "cuboids":
        from mvn_rocm import volumetric
        base, thetas, ref_coords = cases.train_step_cuboid_frames()
        cub = volumetric.build_cuboids(base, 2500.0, 24, thetas, "coco", False, device=device)
        c = cases.train_step_case(scale, coords=ref_coords)
        geometry, coords = cub, cub.coord_volumes()
        assert np.array_equal(coords.cpu().numpy(), ref_coords)
    else:
        c = cases.train_step_case(scale)
        geometry = coords = c["coords"].to(device)
    feat = c["feat"].to(device).requires_grad_(True)
    kps = c["kps"].to(device)
    vol = op.unproject_heatmaps(feat, c["proj"].to(device), geometry, "softmax")
    xyz, vols = op.integrate_tensor_3d_with_coordinates(vol[:, :5], geometry)
    loss = (xyz - kps).abs().mean() + 0.01 * mloss.VolumetricCELoss()(coords, vols, kps, c["validity"].to(device))
    loss.backward()
    ref_loss, ref = cases.train_step_ref(c)
    ours = feat.grad.cpu().numpy()
    per_frame = max_rel_per(ours, ref, 1)
    print(f"scale={scale} {coords_kind}: loss {abs(loss.item() - ref_loss) / abs(ref_loss):.2e}, "
          f"grad_feat per frame {per_frame.max():.2e}")
    assert abs(loss.item() - ref_loss) <= 1e-5 * abs(ref_loss)
    assert (ours[:, :, 5:] == 0).all() and (ref[:, :, 5:] == 0).all()
    assert np.abs(ref).reshape(2, -1).max(1).min() > 0
    assert per_frame.max() <= 1e-4, per_frame
