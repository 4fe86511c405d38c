"""``DeconvHeadEval(project=...)``, ``VolumetricEval.from_projected`` and ``model.VolumetricModelEval`` on
the GPU, on the stand-ins of tests/deconv_project_kit.py: the backbone of
tests/test_gpu_backbone_eval.py (torch.nn modules under the reference's attribute names, 64 x 3 x 4 maps
behind a tiny trunk, M = 6 images) inside a stand-in volumetric model with a random Conv2d(256, 32, 1)
and the randomised stand-in V2VModel(32, 5); B = 2 frames of N = 3 views, 24 x 32 maps, V = 32."""
import copy
import functools

import pytest
import torch

from deconv_project_kit import H4, M, ROWS, W4, stand_in_model
from v2v_kit import assert_same_bits

pytestmark = pytest.mark.gpu

B, N, V = 2, 3, 32
DTYPES = (torch.bfloat16, torch.float32)
DTYPE_IDS = ("bf16", "f32")


@functools.lru_cache(maxsize=None)
def batch():
    """(images (B, N, 3, 12, 16), the synthetic cameras and cuboids), built once."""
    from mvn_rocm import synth
    assert B * N == M
    vb = synth.volumetric_batch(B, n_views=N, channels=8, heatmap=8 * H4, volume=V, seed=3)
    return torch.randn(B, N, 3, 12, 16, generator=torch.Generator().manual_seed(35)), vb


def on_device(device):
    net = copy.deepcopy(stand_in_model()).to(device)
    images, vb = batch()
    return net, images.to(device), vb.proj.to(device), vb.cuboids(device)


def same_outputs(got, want):
    assert len(got) == len(want) == 4
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if g is not None:
            assert_same_bits(g, w)


# ----------------------------------------------------------------------------- the head
@pytest.mark.parametrize("feature_dtype", DTYPES, ids=DTYPE_IDS)
def test_projecting_head_is_the_launches(device, feature_dtype):
    """DeconvHeadEval with ``process_features`` equals the cast-and-permute, two deconv4s2 launches and
    deconv4s2_project made separately, bit for bit."""
    from mvn_rocm import backbone
    net, images, _, _ = on_device(device)
    bb = net.backbone
    with torch.no_grad():
        x4 = bb.trunk(images.view(M, 3, 12, 16))
        head = backbone.DeconvHeadEval.from_reference(bb, device=device, feature_dtype=feature_dtype, heatmaps=False,
                                                      process_features=net.process_features)
        none, f = head(x4)
        dl = bb.deconv_layers
        p = [backbone.fold_deconv_block(dl[3 * i], dl[3 * i + 1], device=device) for i in range(3)]
        conv = net.process_features[0]
        pr = backbone.pack_projection(conv.weight, conv.bias, device=device)
        h = x4.permute(0, 2, 3, 1).to(torch.bfloat16).contiguous()
        h = backbone.deconv4s2(backbone.deconv4s2(h, p[0], "cl"), p[1], "cl")
        f_w = backbone.deconv4s2_project(h, p[2], pr, feature_dtype)
    assert none is None
    assert tuple(f.shape) == (M, ROWS, 8 * H4, 8 * W4) and f.dtype == feature_dtype and f.is_contiguous()
    assert_same_bits(f, f_w)


# ----------------------------------------------------------------------------- VolumetricEval
@pytest.mark.parametrize("feature_dtype", DTYPES, ids=DTYPE_IDS)
def test_forward_is_feature_conv_and_from_projected(device, feature_dtype):
    from mvn_rocm import backbone, model
    net, images, proj, coords = on_device(device)
    be = backbone.BackboneEval.from_reference(net.backbone, device=device, feature_dtype=feature_dtype, heatmaps=False)
    ev = model.VolumetricEval.from_reference(net, device=device, feature_dtype=feature_dtype)
    with torch.no_grad():
        _, f, _, vc = be(images.view(M, 3, 12, 16))
        f, vc = f.view(B, N, *f.shape[1:]), vc.view(B, N, 32)
        for method in ("softmax", "conf_norm"):
            ev.volume_aggregation_method = method
            got = ev(f, proj, coords, vc)
            f32 = model.feature_conv(f, ev.weight, ev.bias, out_dtype=feature_dtype)
            same_outputs(got, ev.from_projected(f32, proj, coords, vc))
    assert tuple(got[0].shape) == (B, 5, 3) and bool(torch.isfinite(got[0]).all())


# ----------------------------------------------------------------------------- VolumetricModelEval
@pytest.mark.parametrize("feature_dtype", DTYPES, ids=DTYPE_IDS)
def test_fused_model_is_the_projecting_backbone_and_from_projected(device, feature_dtype):
    from mvn_rocm import backbone, model
    net, images, proj, coords = on_device(device)
    me = model.VolumetricModelEval.from_reference(net, device=device, feature_dtype=feature_dtype, fused=True)
    be = backbone.BackboneEval.from_reference(net.backbone, device=device, feature_dtype=feature_dtype, heatmaps=False,
                                              process_features=net.process_features)
    ev = model.VolumetricEval.from_reference(net, device=device, feature_dtype=feature_dtype)
    with torch.no_grad():
        got = me(images, proj, coords)
        hm, f, alg, vc = be(images.view(M, 3, 12, 16))
        want = ev.from_projected(f.view(B, N, *f.shape[1:]), proj, coords, vc.view(B, N, 32))
    assert hm is None and alg is None
    assert tuple(got[0].shape) == (B, 5, 3) and bool(torch.isfinite(got[0]).all())
    assert tuple(got[1].shape) == (B, N, ROWS, 8 * H4, 8 * W4) and got[1].dtype == feature_dtype
    same_outputs(got, want)


@pytest.mark.parametrize("feature_dtype", DTYPES, ids=DTYPE_IDS)
def test_unfused_model_is_the_backbone_and_volumetric_eval(device, feature_dtype):
    from mvn_rocm import backbone, model
    net, images, proj, coords = on_device(device)
    me = model.VolumetricModelEval.from_reference(net, device=device, feature_dtype=feature_dtype, fused=False)
    be = backbone.BackboneEval.from_reference(net.backbone, device=device, feature_dtype=feature_dtype, heatmaps=False)
    ev = model.VolumetricEval.from_reference(net, device=device, feature_dtype=feature_dtype)
    with torch.no_grad():
        got = me(images, proj, coords)
        _, f, _, vc = be(images.view(M, 3, 12, 16))
        want = ev(f.view(B, N, *f.shape[1:]), proj, coords, vc.view(B, N, 32))
    same_outputs(got, want)


# ----------------------------------------------------------------------------- the unrounded f32 modules
def test_fused_features_against_the_f32_modules(device):
    """The true semantics: the stand-in's deconv_layers and process_features in f32 on the CPU, against
    the fused 32-channel features and the unfused path's (the head's bf16 maps through feature_conv), both
    as f32: the fused path is held to twice the unfused path's error, max error over max |ref|, the form
    of tests/test_gpu_backbone_eval.py.  Measured on the MI355X: DESIGN.md §4.17."""
    from mvn_rocm import backbone, model
    net_cpu = stand_in_model()
    net, images, _, _ = on_device(device)
    with torch.no_grad():
        x4_cpu = net_cpu.backbone.trunk(batch()[0].view(M, 3, 12, 16))
        ref = net_cpu.process_features(net_cpu.backbone.deconv_layers(x4_cpu))
        x4 = x4_cpu.to(device)                                       # the same layer4 output for both paths
        fused = backbone.DeconvHeadEval.from_reference(net.backbone, device=device, feature_dtype=torch.float32,
                                                       heatmaps=False, process_features=net.process_features)(x4)[1]
        maps = backbone.DeconvHeadEval.from_reference(net.backbone, device=device, heatmaps=False)(x4)[1]
        conv = net.process_features[0]
        unfused = model.feature_conv(maps, conv.weight.detach(), conv.bias.detach(), out_dtype=torch.float32)

    def err(got):
        return float((got.float().cpu() - ref).abs().max()) / float(ref.abs().max())
    ef, eu = err(fused), err(unfused)
    print(f"32-channel features against the f32 modules, max error / max|ref|: fused {ef:.3e}, unfused {eu:.3e}")
    assert ef <= 2 * eu
