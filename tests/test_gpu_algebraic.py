"""The one-call algebraic triangulation (mvn_rocm.multiview.triangulate_from_heatmaps,
csrc/algebraic.hip) on the GPU: against the recorded reference chain, bit for bit against the
existing ops it fuses, its routing, and its backward against the unfused chain's autograd and
a float64 torch-CPU autograd of the same chain."""
import numpy as np
import pytest
import torch

from conftest import assert_bits_equal, max_rel

pytestmark = pytest.mark.gpu

MULT = 100.0


def _f32(t):
    return t.detach().float().cpu().numpy()


def _proj(B, N, J, device, seed=0):
    from mvn_rocm import synth
    return synth.algebraic_batch(B, N, J, seed=seed).proj.to(device)


def _heatmaps(B, N, J, H, W, dtype, device, seed=0, misalign=False):
    """Random maps (unit normal / 25: logits of a few units at multiplier 100).  misalign: a
    contiguous view whose first element is 4 bytes into a 16-byte aligned buffer."""
    g = torch.Generator().manual_seed(seed)
    n = B * N * J * H * W
    off = 0 if not misalign else (1 if dtype is torch.float32 else 2)
    buf = (torch.randn(n + off, generator=g) / 25).to(dtype).to(device)
    hm = buf[off:].view(B, N, J, H, W)
    assert hm.is_contiguous() and hm.data_ptr() % 16 == (4 if misalign else 0)
    return hm


def _conf(B, N, J, device, seed=0):
    g = torch.Generator().manual_seed(seed + 100)
    return (torch.rand(B, N, J, generator=g) * 0.9 + 0.1).to(device)


def _conf_norm_np(conf, B, N, J):
    """Sequential float32 sum in view order, c / s + 1e-5 (triangulation.py:173-174)."""
    c = np.ones((B, N, J), np.float32) if conf is None else _f32(conf)
    s = c[:, 0].copy()
    for v in range(1, N):
        s = s + c[:, v]
    with np.errstate(invalid="ignore", divide="ignore"):
        return c / s[:, None] + np.float32(1e-5)


def _check_against_ops(hm, proj, conf, image_shape, softmax, return_heatmaps, out_dtype=None):
    """fused=True against the existing ops, bit for bit."""
    from mvn_rocm import multiview, op
    B, N, J, H, W = hm.shape
    xyz, kp2d, maps, cn = multiview.triangulate_from_heatmaps(
        hm, proj, conf, image_shape=image_shape, heatmap_multiplier=MULT, heatmap_softmax=softmax,
        return_heatmaps=return_heatmaps, out_dtype=out_dtype, fused=True)
    xy_ref, maps_ref = op.integrate_tensor_2d(hm.view(B * N, J, H, W), softmax, multiplier=MULT,
                                              return_heatmaps=return_heatmaps, out_dtype=out_dtype)
    scale = torch.tensor([image_shape[1] / W, image_shape[0] / H], dtype=torch.float32, device=hm.device)
    assert_bits_equal(_f32(kp2d), _f32(xy_ref.view(B, N, J, 2) * scale))
    if return_heatmaps:
        assert maps.dtype == maps_ref.dtype and tuple(maps.shape) == (B, N, J, H, W)
        assert_bits_equal(_f32(maps), _f32(maps_ref.view(B, N, J, H, W)))
    else:
        assert maps is None
    assert_bits_equal(_f32(cn), _conf_norm_np(conf, B, N, J))
    assert_bits_equal(_f32(xyz), _f32(multiview.triangulate_batch_of_points(proj, kp2d, cn)))
    return xyz, kp2d, maps, cn


# ----------------------------------------------------------------------------- reference chain
def test_fused_chain_matches_reference_model(golden, device):
    """AlgebraicTriangulationNet.forward as recorded from the reference (chains.npz: B = 2,
    N = 4, J = 17, 96^2, multiplier 100), the bars of test_algebraic_chain_matches_reference_model;
    the normalised confidences bit for bit (a sequential float32 sum is torch's for N <= 4)."""
    from mvn_rocm import multiview
    d = golden("chains.npz")
    hm = torch.from_numpy(d["alg_heatmaps"].astype(np.float32)).to(device)
    xyz, kp2d, maps, cn = multiview.triangulate_from_heatmaps(
        hm, torch.from_numpy(d["alg_proj"]).to(device), torch.from_numpy(d["alg_conf"]).to(device),
        image_shape=(384, 384), heatmap_multiplier=float(d["alg_multiplier"]), fused=True)
    e2, e3, e3f = max_rel(_f32(kp2d), d["alg_kp2d64"]), max_rel(_f32(xyz), d["alg_kp3d64"]), max_rel(_f32(xyz), d["alg_kp3d"])
    print(f"kp2d vs f64 {e2:.3e}  kp3d vs f64 {e3:.3e}  kp3d vs f32 reference {e3f:.3e}")
    assert e2 <= 1e-5
    assert e3 <= 1e-4
    assert e3f <= 1e-3
    assert_bits_equal(_f32(cn), d["alg_conf_norm"])
    assert tuple(maps.shape) == hm.shape and abs(float(maps.sum()) - 2 * 4 * 17) <= 1e-2


# ----------------------------------------------------------------------------- against the existing ops
# (B, N, J, H, W, image_shape, misaligned): every view-group count and round pattern, both map
# bodies, partial runs, fewer pixels than threads, inexact scales
SHAPES = [
    (1, 2, 1, 96, 96, (400, 400), False),       # two groups
    (3, 3, 17, 16, 16, (50, 70), False),        # four groups, one idle; fewer pixels than threads
    (1, 4, 17, 96, 96, (400, 400), False),      # config 1, inexact scale
    (1, 5, 3, 112, 108, (400, 300), False),     # second round with one live group; last run partial
    (3, 8, 1, 17, 23, (100, 100), False),       # two full rounds; W % 4 != 0: three-pass body
    (1, 4, 1, 128, 128, (384, 384), False),     # > 12,288 px: three-pass body
    (1, 1, 2, 16, 16, (64, 64), False),         # a single view: one group
    (1, 4, 2, 96, 96, (400, 400), True),        # maps 4-byte but not 16-byte aligned: three-pass body
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B{}N{}J{}_{}x{}{}".format(*s[:5], "_misaligned" if s[6] else ""))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_fused_equals_existing_ops_bit_for_bit(device, shape, dtype):
    B, N, J, H, W, image_shape, misalign = shape
    hm = _heatmaps(B, N, J, H, W, dtype, device, seed=N, misalign=misalign)
    proj, conf = _proj(B, N, J, device), _conf(B, N, J, device)
    for softmax in (True, False):
        for return_heatmaps in (True, False):
            _check_against_ops(hm, proj, conf, image_shape, softmax, return_heatmaps)
    if dtype is torch.bfloat16:
        _check_against_ops(hm, proj, conf, image_shape, True, True, out_dtype=torch.float32)


@pytest.mark.parametrize("N", [3, 4, 5])
def test_confidence_cases(device, N):
    """No confidences (all ones), and one view's confidence 0 (that view drops out of the DLT
    but for the 1e-5)."""
    B, J, H, W = 3, 17, 16, 16
    hm, proj = _heatmaps(B, N, J, H, W, torch.float32, device, seed=7), _proj(B, N, J, device)
    _, _, _, cn = _check_against_ops(hm, proj, None, (64, 64), True, True)
    assert_bits_equal(_f32(cn), np.full((B, N, J), np.float32(1) / np.float32(N) + np.float32(1e-5), np.float32))
    conf = _conf(B, N, J, device)
    conf[:, 1] = 0
    _, _, _, cn = _check_against_ops(hm, proj, conf, (64, 64), True, False)
    assert_bits_equal(_f32(cn)[:, 1], np.full((B, J), 1e-5, np.float32))


def _assert_same_with_nans(a, b):
    a, b = _f32(a), _f32(b)
    assert (np.isnan(a) == np.isnan(b)).all()
    assert_bits_equal(np.nan_to_num(a, nan=0.0), np.nan_to_num(b, nan=0.0))


def test_all_zero_confidences_of_one_joint(device):
    """c / 0 = NaN: in exactly that joint and its confidences, position by position as the
    composition of the existing ops gives."""
    from mvn_rocm import multiview
    B, N, J, H, W = 2, 4, 5, 16, 16
    hm, proj, conf = _heatmaps(B, N, J, H, W, torch.float32, device), _proj(B, N, J, device), _conf(B, N, J, device)
    conf[1, :, 3] = 0
    kw = dict(image_shape=(64, 64), heatmap_multiplier=MULT)
    fused = multiview.triangulate_from_heatmaps(hm, proj, conf, fused=True, **kw)
    composed = multiview.triangulate_from_heatmaps(hm, proj, conf, fused=False, **kw)
    for a, b in zip(fused, composed):
        _assert_same_with_nans(a, b)
    xyz, kp2d, maps, cn = (_f32(t) for t in fused)
    nan_x, nan_c = np.zeros((B, J), bool), np.zeros((B, N, J), bool)
    nan_x[1, 3], nan_c[1, :, 3] = True, True
    assert (np.isnan(xyz).all(axis=-1) == nan_x).all() and (np.isnan(xyz).any(axis=-1) == nan_x).all()
    assert (np.isnan(cn) == nan_c).all()
    assert not np.isnan(kp2d).any() and not np.isnan(maps).any()


@pytest.mark.parametrize("H,W", [(16, 16), (17, 23)], ids=["register", "three_pass"])
def test_nan_pixel_stays_in_its_joint(device, H, W):
    from mvn_rocm import multiview
    B, N, J = 2, 3, 5
    hm, proj, conf = _heatmaps(B, N, J, H, W, torch.float32, device), _proj(B, N, J, device), _conf(B, N, J, device)
    hm[1, 2, 4, H // 2, 3] = float("nan")
    kw = dict(image_shape=(64, 64), heatmap_multiplier=MULT)
    fused = multiview.triangulate_from_heatmaps(hm, proj, conf, fused=True, **kw)
    composed = multiview.triangulate_from_heatmaps(hm, proj, conf, fused=False, **kw)
    for a, b in zip(fused, composed):
        _assert_same_with_nans(a, b)
    xyz, kp2d, maps, cn = (_f32(t) for t in fused)
    nan_x, nan_k = np.zeros((B, J), bool), np.zeros((B, N, J), bool)
    nan_x[1, 4], nan_k[1, 2, 4] = True, True
    assert (np.isnan(xyz).any(axis=-1) == nan_x).all()
    assert (np.isnan(kp2d).any(axis=-1) == nan_k).all()
    assert (np.isnan(maps).any(axis=(-1, -2)) == nan_k).all()
    assert not np.isnan(cn).any()


@pytest.mark.parametrize("H,W", [(16, 16), (17, 23)], ids=["register", "three_pass"])
def test_relu_nan_pixel_follows_torch(device, H, W):
    """relu mode (heatmap_softmax=False): torch's relu keeps a NaN (op.py:27), so the map's
    (x, y) are NaN and the returned map holds the NaN at its pixel — op.integrate_tensor_2d on
    both map bodies against torch on the CPU (float64 on the float32 products), then the fused
    call against the composed ops."""
    from mvn_rocm import multiview, op
    from oracle import restate_torch
    B, N, J = 2, 3, 5
    hm, proj, conf = _heatmaps(B, N, J, H, W, torch.float32, device), _proj(B, N, J, device), _conf(B, N, J, device)
    hm[1, 2, 4, H // 2, 3] = float("nan")
    bad = np.zeros((B * N, J), bool)
    bad[1 * N + 2, 4] = True
    xy, maps = op.integrate_tensor_2d(hm.view(B * N, J, H, W), False, multiplier=MULT)
    scaled = (hm.cpu().view(B * N, J, H, W) * torch.tensor(MULT, dtype=torch.float32)).double()
    rxy, rmaps = restate_torch.integrate_tensor_2d(scaled, False)
    xy, maps, rxy, rmaps = _f32(xy), _f32(maps), rxy.numpy(), rmaps.numpy()
    assert (np.isnan(rxy).all(axis=-1) == bad).all() and (np.isnan(rxy).any(axis=-1) == bad).all()
    assert (np.isnan(xy) == np.isnan(rxy)).all()
    assert max_rel(xy[~bad], rxy[~bad]) <= 1e-5
    assert np.isnan(rmaps).sum() == 1 and (np.isnan(maps) == np.isnan(rmaps)).all()
    assert_bits_equal(np.nan_to_num(maps, nan=0.0), np.nan_to_num(rmaps, nan=0.0).astype(np.float32))
    kw = dict(image_shape=(64, 64), heatmap_multiplier=MULT, heatmap_softmax=False)
    fused = multiview.triangulate_from_heatmaps(hm, proj, conf, fused=True, **kw)
    composed = multiview.triangulate_from_heatmaps(hm, proj, conf, fused=False, **kw)
    for a, b in zip(fused, composed):
        _assert_same_with_nans(a, b)
    xyz, kp2d, fmaps, cn = (_f32(t) for t in fused)
    nan_x = np.zeros((B, J), bool)
    nan_x[1, 4] = True
    assert (np.isnan(xyz).any(axis=-1) == nan_x).all()
    assert (np.isnan(kp2d).any(axis=-1).reshape(B * N, J) == bad).all()
    assert (np.isnan(fmaps).reshape(B * N, J, -1).sum(-1) == bad).all()
    assert not np.isnan(cn).any()


def test_more_views_than_the_kernel_takes(device):
    """N = 33: Python routes around the kernel (MVN_ERR_SHAPE in the C ABI), whatever `fused`."""
    from mvn_rocm import multiview
    B, N, J, H, W = 1, 33, 2, 16, 16
    hm, proj, conf = _heatmaps(B, N, J, H, W, torch.float32, device), _proj(B, N, J, device), _conf(B, N, J, device)
    kw = dict(image_shape=(64, 64), heatmap_multiplier=MULT)
    composed = multiview.triangulate_from_heatmaps(hm, proj, conf, fused=False, **kw)
    for fused in (True, None):
        for a, b in zip(multiview.triangulate_from_heatmaps(hm, proj, conf, fused=fused, **kw), composed):
            assert_bits_equal(_f32(a), _f32(b))


# ----------------------------------------------------------------------------- routing
def test_unfused_path_is_the_composition_of_the_existing_ops(device):
    from mvn_rocm import multiview, op
    B, N, J, H, W = 2, 4, 5, 16, 16
    hm, proj, conf = _heatmaps(B, N, J, H, W, torch.float32, device), _proj(B, N, J, device), _conf(B, N, J, device)
    xyz, kp2d, maps, cn = multiview.triangulate_from_heatmaps(hm, proj, conf, image_shape=(50, 70),
                                                              heatmap_multiplier=MULT, fused=False)
    xy, m = op.integrate_tensor_2d(hm.view(B * N, J, H, W), True, multiplier=MULT)
    xy = xy.view(B, N, J, 2)
    c = conf / conf.sum(dim=1, keepdim=True) + 1e-5
    k = torch.stack([xy[..., 0] * (70 / W), xy[..., 1] * (50 / H)], dim=-1)
    assert_bits_equal(_f32(kp2d), _f32(k))
    assert_bits_equal(_f32(maps), _f32(m.view(B, N, J, H, W)))
    assert_bits_equal(_f32(cn), _f32(c))
    assert_bits_equal(_f32(xyz), _f32(multiview.triangulate_batch_of_points(proj, k, c)))


def test_routing_threshold(device, monkeypatch):
    """fused=None: the kernel up to FUSED_MAX_POINTS points (B * J), the composition above;
    either way the tuple of the forced paths (N = 4: the same bits on both)."""
    from mvn_rocm import _ops, multiview
    launches = []
    eager = _ops.algebraic_triangulate.eager
    monkeypatch.setattr(_ops.algebraic_triangulate, "eager", lambda *a: (launches.append(1), eager(*a))[1])
    monkeypatch.setattr(multiview, "FUSED_MAX_POINTS", 10)
    N, H, W = 4, 16, 16
    kw = dict(image_shape=(50, 70), heatmap_multiplier=MULT)
    for B, J, want in ((2, 5, 1), (1, 11, 0), (3, 5, 0)):
        hm, proj, conf = _heatmaps(B, N, J, H, W, torch.float32, device), _proj(B, N, J, device), _conf(B, N, J, device)
        del launches[:]
        auto = multiview.triangulate_from_heatmaps(hm, proj, conf, **kw)
        assert len(launches) == want, (B, J)
        for fused in (True, False):
            for a, b in zip(auto, multiview.triangulate_from_heatmaps(hm, proj, conf, fused=fused, **kw)):
                assert_bits_equal(_f32(a), _f32(b))


def test_default_threshold_is_positive():
    from mvn_rocm import multiview
    assert multiview.FUSED_MAX_POINTS >= 17          # config 1 (B = 1, J = 17) takes the kernel


# ----------------------------------------------------------------------------- backward
def _blob_case(N, device, use_conf):
    """B = 2, J = 5, 32 x 32 maps, multiplier 100: a blob per (b, v, j) around the joint's
    projection (384^2 image, clipped into the map), logits up to ~10."""
    from mvn_rocm import synth
    B, J, H, W = 2, 5, 32, 32
    ab = synth.algebraic_batch(B, N, J, seed=3)
    c = (ab.points / (384 / W)).clamp(3.0, W - 4.0)                   # (B, N, J, 2)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    d2 = (xs - c[..., 0, None, None]) ** 2 + (ys - c[..., 1, None, None]) ** 2
    g = torch.Generator().manual_seed(5)
    hm = 0.1 * torch.exp(-d2 / (2 * 2.5 ** 2)) + 0.002 * torch.randn(B, N, J, H, W, generator=g)
    conf = (torch.rand(B, N, J, generator=g) * 0.9 + 0.1) if use_conf else None
    gx = torch.randn(B, J, 3, generator=g)
    gm = torch.randn(B, N, J, H, W, generator=g)
    return hm, ab.proj, conf, gx, gm


def _gpu_grads(case, device, fused, through_maps):
    from mvn_rocm import multiview
    hm, proj, conf, gx, gm = case
    hm = hm.to(device).requires_grad_()
    conf = None if conf is None else conf.to(device).requires_grad_()
    xyz, kp2d, maps, cn = multiview.triangulate_from_heatmaps(hm, proj.to(device), conf, image_shape=(384, 384),
                                                              heatmap_multiplier=MULT, fused=fused)
    loss = (xyz * gx.to(device)).sum()
    if through_maps:
        loss = loss + (maps * gm.to(device)).sum()
    loss.backward()
    return hm.grad.cpu().numpy(), (None if conf is None else conf.grad.cpu().numpy())


def _f64_grads(case, through_maps):
    """float64 torch-CPU autograd of triangulation.py:164-191 from the oracle's restatements."""
    from oracle import restate_torch as rt
    hm, proj, conf, gx, gm = case
    B, N, J, H, W = hm.shape
    hm = hm.double().requires_grad_()
    c = torch.ones(B, N, J, dtype=torch.float64) if conf is None else conf.double().requires_grad_()
    xy, maps = rt.integrate_tensor_2d(hm.view(B * N, J, H, W) * MULT, True)
    xy = xy.view(B, N, J, 2)
    cn = c / c.sum(dim=1, keepdim=True) + 1e-5
    kp2d = torch.stack([xy[..., 0] * (384 / W), xy[..., 1] * (384 / H)], dim=-1)
    xyz = rt.triangulate_batch_of_points(proj.double(), kp2d, cn)
    loss = (xyz.double() * gx.double()).sum()
    if through_maps:
        loss = loss + (maps.view(B, N, J, H, W) * gm.double()).sum()
    loss.backward()
    return hm.grad.numpy(), (None if conf is None else c.grad.numpy())


@pytest.fixture(scope="module")
def backward_refs():
    cache = {}

    def get(N, use_conf, through_maps):
        key = (N, use_conf, through_maps)
        if key not in cache:
            cache[key] = _f64_grads(_blob_case(N, None, use_conf), through_maps)
        return cache[key]
    return get


@pytest.mark.parametrize("through_maps", [False, True], ids=["joints", "joints_and_maps"])
@pytest.mark.parametrize("use_conf", [True, False], ids=["conf", "noconf"])
@pytest.mark.parametrize("N", [4, 3])
def test_backward_matches_unfused_chain_and_float64(device, backward_refs, N, use_conf, through_maps):
    """Gradients of the fused op: within 1e-5 (max-rel per tensor, the DLT backward's bar) of the
    unfused chain's autograd on the GPU, and no farther than twice the unfused chain's own
    distance from the float64 CPU autograd of the same chain (both run the same backward
    kernels on the same saved tensors).  Measured on an MI355X:
    see the table there."""
    case = _blob_case(N, device, use_conf)
    fused = _gpu_grads(case, device, True, through_maps)
    unfused = _gpu_grads(case, device, False, through_maps)
    ref = backward_refs(N, use_conf, through_maps)
    for name, f, u, r in zip(("grad_heatmaps", "grad_confidences"), fused, unfused, ref):
        if f is None:
            assert u is None and name == "grad_confidences" and not use_conf
            continue
        assert np.isfinite(f).all() and np.abs(r).max() > 0
        d, ef, eu = max_rel(f, u), max_rel(f, r), max_rel(u, r)
        print(f"N={N} conf={use_conf} maps={through_maps} {name}: fused vs unfused {d:.3e}  "
              f"fused vs f64 {ef:.3e}  unfused vs f64 {eu:.3e}")
        assert d <= 1e-5
        assert ef <= 2 * eu
