"""model.VolumetricEval on the MI355X: the volumetric model from the backbone's
feature maps to the joints.  A stand-in net (test_feature_conv_api.StandInNet: a random
Conv2d(256, 32, 1) and the randomised stand-in V2VModel(32, 5)), B = 2 frames of N = 3 views, 24 x 24
maps, V = 32, synth cameras and cuboids."""
import functools

import pytest
import torch
import torch.nn.functional as F

from test_feature_conv_api import stand_in_net
from v2v_kit import E2E_MULT, assert_same_bits

pytestmark = pytest.mark.gpu

B, N, CIN, HM, V, J = 2, 3, 256, 24, 32, 5


def blob_features(vb, seed):
    """Backbone-like maps: per frame J points inside the cuboid; channel c of every view holds a 2D
    Gaussian (height 5, sigma 1.5 pixels) at the projection of point c mod J, over 0.1 x unit noise.
    Any 1x1 convolution of them is a mixture of the same J blobs, their unprojection J blobs in the
    volume (largest voxel 10.7 here, as the blobs of height 10 of v2v_kit.e2e_case), which
    keeps the soft-argmax well conditioned under that test's multiplier: every joint's largest logit
    is 13 or more above its mean on the CPU reference."""
    g = torch.Generator().manual_seed(seed)
    feats = 0.1 * torch.randn(B, N, CIN, HM, HM, generator=g)
    ys, xs = torch.meshgrid(torch.arange(HM).float(), torch.arange(HM).float(), indexing="ij")
    for b in range(B):
        idx = torch.randint(V // 4, 3 * V // 4, (J, 3), generator=g)
        pts = vb.coords[b, idx[:, 0], idx[:, 1], idx[:, 2]]                       # (J, 3) world coordinates
        for v in range(N):
            h = torch.cat([pts, torch.ones(J, 1)], dim=1) @ vb.proj[b, v].T       # (J, 3) homogeneous pixels
            u, w = h[:, 0] / h[:, 2], h[:, 1] / h[:, 2]
            blobs = 5.0 * torch.exp(-((xs[None] - u[:, None, None]) ** 2 + (ys[None] - w[:, None, None]) ** 2)
                                     / (2 * 1.5 ** 2))
            feats[b, v] += blobs[torch.arange(CIN) % J]
    return feats


@functools.lru_cache(maxsize=None)
def case():
    """(synthetic batch with blob-like feature maps, stand-in net, vol_confidences (B, N, 32) > 0),
    built once."""
    from mvn_rocm import synth
    vb = synth.volumetric_batch(B, n_views=N, channels=8, heatmap=HM, volume=V, seed=3)
    vb.features = blob_features(vb, seed=3)
    net = stand_in_net(seed=2025, J=J, multiplier=E2E_MULT)
    conf = 0.25 + torch.rand(B, N, 32, generator=torch.Generator().manual_seed(8))
    return vb, net, conf


@functools.lru_cache(maxsize=None)
def modules(device, feature_dtype):
    """(VolumetricEval.from_reference, an independent V2VEval of the same volume_net)."""
    from mvn_rocm import model, v2v
    _, net, _ = case()
    return (model.VolumetricEval.from_reference(net, device=device, feature_dtype=feature_dtype),
            v2v.V2VEval.from_reference(net.volume_net, device=device, half_res="kernels", deep="kernels"))


def coordinates(vb, device, kind):
    return vb.cuboids(device) if kind == "cuboids" else vb.coords.to(device)


@pytest.mark.parametrize("feature_dtype", (torch.bfloat16, torch.float32), ids=("bf16", "f32"))
@pytest.mark.parametrize("kind", ("cuboids", "tensor"))
@pytest.mark.parametrize("method", ("softmax", "sum", "conf", "conf_norm"))
def test_forward_is_the_composition(device, method, kind, feature_dtype):
    """VolumetricEval.forward equals, bit for bit, feature_conv, unproject_channels_last and
    V2VEval.forward called one after the other with the same arguments."""
    from mvn_rocm import model, v2v
    vb, net, conf = case()
    ev, v2veval = modules(device, feature_dtype)
    ev.volume_aggregation_method = method
    conv = net.process_features[0]
    feats, proj, vc = vb.features.to(device), vb.proj.to(device), conf.to(device)
    coords = coordinates(vb, device, kind)
    with torch.no_grad():
        kp, f32, vols, vc_out = ev(feats, proj, coords, vc)
        f_w = model.feature_conv(feats, conv.weight.detach().to(device), conv.bias.detach().to(device),
                                 out_dtype=feature_dtype)
        vc_w = vc / vc.sum(dim=1, keepdim=True) if method == "conf_norm" else vc      # triangulation.py:268-269
        vol = v2v.unproject_channels_last(f_w, proj, coords, method, out_dtype=torch.bfloat16, vol_confidences=vc_w)
        kp_w, vols_w = v2veval(vol, coords, net.volume_multiplier, net.volume_softmax)
    assert tuple(kp.shape) == (B, J, 3) and tuple(vols.shape) == (B, J, V, V, V)
    assert tuple(f32.shape) == (B, N, 32, HM, HM) and f32.dtype == feature_dtype
    assert bool(torch.isfinite(kp).all())
    assert_same_bits(f32, f_w)
    assert_same_bits(kp, kp_w)
    assert_same_bits(vols, vols_w)
    assert torch.equal(vc_out, vc_w)
    if method == "conf_norm":
        assert torch.allclose(vc_out.sum(dim=1), torch.ones(B, 32, device=device), atol=1e-6)
        assert not torch.equal(vc_out, vc)
    else:
        assert vc_out is vc


def test_against_the_f32_modules(device):
    """The true semantics in one run: F.conv2d, the C oracle's unprojection, the f32 stand-in V2V and
    torch's soft-argmax on the CPU, against (a) VolumetricEval and (b) the path it replaces
    (F.conv2d on the GPU in f32, .to(bfloat16), unproject_channels_last, the same V2VEval).  The two
    differ in the conv's summation order (about 1e-6) before the same bf16 rounding, so (a) is held
    to twice (b)'s error, the factor of DESIGN.md §4.13 and §4.14 for bf16 roundings that flip.
    Measured on the MI355X (softmax aggregation, multiplier 10): VolumetricEval trunk
    8.119e-3 of max|ref|, joints 4.745e-3 of the 2500 mm side; the four-call path 8.119e-3 and 6.563e-3."""
    from mvn_rocm import synth, v2v
    from oracle import capi, restate_torch
    vb, net, _ = case()
    ev, v2veval = modules(device, torch.bfloat16)
    ev.volume_aggregation_method = "softmax"
    conv, m, mult = net.process_features[0], net.volume_net, net.volume_multiplier
    with torch.no_grad():
        f_ref = F.conv2d(vb.features.view(B * N, CIN, HM, HM), conv.weight, conv.bias).view(B, N, 32, HM, HM)
        vol_ref = torch.from_numpy(capi.unproject(f_ref.numpy(), vb.proj.numpy(), vb.coords.numpy(), "softmax"))
        t_ref = m.back_layers[0](m.encoder_decoder(m.front_layers(vol_ref)))
        logits = m.output_layer(m.back_layers[2](m.back_layers[1](t_ref)))
        kp_ref, _ = restate_torch.integrate_tensor_3d_with_coordinates(logits * mult, vb.coords, softmax=True)

        feats, proj, coords = vb.features.to(device), vb.proj.to(device), vb.cuboids(device)
        kp_a, f_a, _, _ = ev(feats, proj, coords)
        t_a = ev.v2v.trunk(v2v.unproject_channels_last(f_a, proj, coords, "softmax"))
        f_b = F.conv2d(feats.view(B * N, CIN, HM, HM), conv.weight.to(device), conv.bias.to(device))
        vol_b = v2v.unproject_channels_last(f_b.view(B, N, 32, HM, HM).to(torch.bfloat16), proj, coords, "softmax")
        t_b = v2veval.trunk(vol_b)
        kp_b, _ = v2veval(vol_b, coords, mult, True)
    den = float(t_ref.abs().max())
    # the premise, as in test_gpu_v2v_res3d: every joint's largest logit stands well above its mean
    peak = float(((logits * mult).amax(dim=(2, 3, 4)) - (logits * mult).mean(dim=(2, 3, 4))).min())
    print(f"peak logit above the mean, smallest over the joints: {peak:.1f}")
    assert peak > 4.0

    def errors(t, kp):
        return (float((t.permute(0, 4, 1, 2, 3).float().cpu() - t_ref).abs().max()) / den,
                float((kp.cpu() - kp_ref).abs().max()) / synth.CUBOID_SIDE)
    (trunk_a, joints_a), (trunk_b, joints_b) = errors(t_a, kp_a), errors(t_b, kp_b)
    print(f"VolumetricEval against the f32 modules: trunk {trunk_a:.3e} of max|ref|, joints {joints_a:.3e} of the "
          f"side; the four-call path with F.conv2d: trunk {trunk_b:.3e}, joints {joints_b:.3e}")
    assert trunk_a <= 2 * trunk_b
    assert joints_a <= 2 * joints_b


def test_autograd_recorded_inputs_are_refused(device):
    vb, _, conf = case()
    ev, _ = modules(device, torch.bfloat16)
    ev.volume_aggregation_method = "conf"
    feats, proj, vc = vb.features.to(device), vb.proj.to(device), conf.to(device)
    coords = vb.cuboids(device)
    with pytest.raises(RuntimeError, match="inference-only"):
        ev(feats.clone().requires_grad_(), proj, coords, vc)
    with pytest.raises(RuntimeError, match="inference-only"):
        ev(feats, proj, coords, vc.clone().requires_grad_())
    with torch.no_grad():
        kp, _, _, _ = ev(feats.clone().requires_grad_(), proj, coords, vc)
    assert not kp.requires_grad and tuple(kp.shape) == (B, J, 3)
