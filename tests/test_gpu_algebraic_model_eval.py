"""``model.AlgebraicModelEval`` on the GPU: images to 3-D joints in one call equals
``multiview.triangulate_from_heatmaps`` applied by hand to ``BackboneEval``'s outputs, bit for bit, with and
without confidences, with and without the softmax, at both extremes of the ``trunk`` / ``stem`` / ``confidences``
switches; B = 2 frames of N = 3 views, 64 x 96 images, the stand-ins of tests/confidence_kit.py."""
import copy
import functools

import pytest
import torch
from torch import nn

from confidence_kit import IMAGE, StandInAlgebraicModel, stand_in_backbone
from v2v_kit import assert_same_bits

pytestmark = pytest.mark.gpu

B, N, J = 2, 3, 17
SWITCHES = {"torch": dict(trunk="torch", stem="torch", confidences="torch"),
            "kernels": dict(trunk="kernels", stem="kernels", confidences="kernels")}


@functools.lru_cache(maxsize=None)
def batch():
    from mvn_rocm import synth
    images = torch.randn(B, N, 3, *IMAGE, generator=torch.Generator().manual_seed(91))
    return images, synth.algebraic_batch(B, N, J, seed=2).proj.float()


def on_device(device, use_confidences, softmax, multiplier, with_alg=True):
    net = StandInAlgebraicModel(copy.deepcopy(stand_in_backbone(J, with_alg)).to(device), use_confidences, softmax, multiplier)
    images, proj = batch()
    return net, images.to(device), proj.to(device)


@pytest.mark.parametrize("switches", SWITCHES)
@pytest.mark.parametrize("use_confidences, softmax, multiplier", ((True, True, 100.0), (False, True, 100.0), (True, False, 1.0),
                                                                   (False, False, 100.0)),
                         ids=("conf_softmax_x100", "ones_softmax_x100", "conf_relu_x1", "ones_relu_x100"))
def test_forward_is_the_backbone_and_triangulate_from_heatmaps(device, switches, use_confidences, softmax, multiplier):
    from mvn_rocm import backbone, model, multiview
    kw = SWITCHES[switches]
    net, images, proj = on_device(device, use_confidences, softmax, multiplier)
    me = model.AlgebraicModelEval.from_reference(net, device=device, **kw)
    assert isinstance(me.backbone, backbone.BackboneEval) and me.backbone.head.heatmaps
    seen = []
    hook = me.backbone.register_forward_hook(lambda mod, args, out: seen.append((args[0], out)))
    with torch.no_grad():
        got = me(images, proj)
        hook.remove()
        (x_in, (hm, _, alg, _)), = seen                              # this run's BackboneEval outputs
        want = multiview.triangulate_from_heatmaps(hm, proj, alg if use_confidences else None, image_shape=IMAGE,
                                                   heatmap_multiplier=multiplier, heatmap_softmax=softmax)
        if switches == "kernels":
            # nothing of torch's is left, and the kernels repeat themselves bit for bit: a BackboneEval built
            # apart gives the same outputs (torch's own convolutions need not: tests/test_gpu_confidence_head_eval.py)
            assert not any(isinstance(m, (nn.Conv2d, nn.Linear, nn.ConvTranspose2d)) for m in me.modules())
            be = backbone.BackboneEval.from_reference(net.backbone, device=device, heatmaps=True, **kw)
            hm_b, _, alg_b, _ = be(images.view(B * N, 3, *IMAGE))
            assert_same_bits(hm_b, hm)
            assert_same_bits(alg_b, alg)
    assert tuple(x_in.shape) == (B * N, 3, *IMAGE) and x_in.data_ptr() == images.data_ptr()
    assert tuple(hm.shape) == (B * N, J, *IMAGE) and tuple(alg.shape) == (B * N, J)
    assert len(got) == len(want) == 4
    for g, w in zip(got, want):
        assert_same_bits(g, w)
    kp3d, kp2d, maps, conf = got
    assert tuple(kp3d.shape) == (B, J, 3) and kp3d.dtype == torch.float32
    assert tuple(kp2d.shape) == (B, N, J, 2) and kp2d.dtype == torch.float32
    assert tuple(maps.shape) == (B, N, J, *IMAGE) and maps.dtype == torch.float32      # the stand-in's maps are image-sized
    assert tuple(conf.shape) == (B, N, J) and conf.dtype == torch.float32
    if softmax:                                                      # without it a joint whose map is all <= 0 is 0 / 0
        assert bool(torch.isfinite(kp3d).all()) and bool(torch.isfinite(kp2d).all())
    if not use_confidences:                                          # the reference's all ones, normalised
        ones = torch.ones(B, N, J, device=device)
        assert_same_bits(conf, ones / ones.sum(dim=1, keepdim=True) + 1e-5)
    else:
        assert conf.unique().numel() > 1


def test_a_backbone_without_the_head_runs_without_confidences(device):
    from mvn_rocm import backbone, model, multiview
    net, images, proj = on_device(device, False, True, 100.0, with_alg=False)
    me = model.AlgebraicModelEval.from_reference(net, device=device, **SWITCHES["kernels"])
    assert me.backbone.alg_confidences is None
    be = backbone.BackboneEval.from_reference(net.backbone, device=device, **SWITCHES["kernels"])
    with torch.no_grad():
        got = me(images, proj)
        hm, _, alg, _ = be(images.view(B * N, 3, *IMAGE))
        want = multiview.triangulate_from_heatmaps(hm, proj, None, image_shape=IMAGE, heatmap_multiplier=100.0)
    assert alg is None
    for g, w in zip(got, want):
        assert_same_bits(g, w)


def test_an_input_that_requires_grad_raises(device):
    from mvn_rocm import model
    net, images, proj = on_device(device, True, True, 100.0)
    me = model.AlgebraicModelEval.from_reference(net, device=device)
    with pytest.raises(RuntimeError, match="inference-only"):
        me(images.clone().requires_grad_(True), proj)
    with pytest.raises(RuntimeError, match=r"\(B, N, 3, H, W\)"):
        me(images.view(B * N, 3, *IMAGE), proj)
