"""``resnet.StemEval`` inside ``TrunkEval``, ``BackboneEval`` and ``VolumetricModelEval`` (``stem="kernels"``) on the
GPU, on the stand-in backbone of tests/bottleneck_kit.py: M = 3 images of 3 x 40 x 56, a stem map
of 10 x 14, then the maps of tests/test_gpu_trunk_eval.py."""
import copy

import pytest
import torch

from bottleneck_kit import TRUNK_COUT, TRUNK_M, stand_in_backbone, stand_in_trunk_model, trunk_images
from deconv_kit import nchw
from stem_kit import check_bound, cpu_stem
from v2v_kit import assert_same_bits

pytestmark = pytest.mark.gpu


def on_device(device):
    return copy.deepcopy(stand_in_backbone()).to(device), trunk_images().to(device)


def test_forward_is_the_stem_launch_and_the_block_launches(device, monkeypatch):
    """TrunkEval(stem="kernels").forward equals the stem launch and the 18 block launches made one by one, bit for
    bit; the first block reads the stem's output itself (no cast-and-permute pass, no copy)."""
    from mvn_rocm import resnet
    net, images = on_device(device)
    trunk = resnet.TrunkEval.from_reference(net, device=device, stem="kernels")
    assert isinstance(trunk.stem, resnet.StemEval) and len(trunk.blocks) == 6
    assert not any(isinstance(m, torch.nn.Conv2d) for m in trunk.modules())
    seen = {}
    stem_launch, first_block = resnet.stem, type(trunk.blocks[0]).forward

    def spy_stem(*args):
        seen["stem_out"] = stem_launch(*args)
        return seen["stem_out"]

    def spy_block(self, x_cl):
        seen.setdefault("block_in", []).append(x_cl)
        return first_block(self, x_cl)
    monkeypatch.setattr(resnet, "stem", spy_stem)
    monkeypatch.setattr(type(trunk.blocks[0]), "forward", spy_block)
    y = trunk(images)                                             # no grad mode needed: nothing of it has parameters
    monkeypatch.undo()
    assert seen["block_in"][0] is seen["stem_out"] and seen["block_in"][0].data_ptr() == seen["stem_out"].data_ptr()
    assert len(seen["block_in"]) == 6
    h = resnet.stem(images, *resnet.fold_stem(net.conv1, net.bn1, net.relu, net.maxpool, device=device))
    assert tuple(h.shape) == (TRUNK_M, 10, 14, 64) and h.dtype == torch.bfloat16 and h.is_contiguous()
    assert_same_bits(seen["stem_out"], h)
    launches = 0
    for block in net.blocks():
        p = resnet.fold_bottleneck(block, device=device)
        a = resnet.conv1x1(h, *p.conv1)
        b = resnet.conv3x3(a, *p.conv2, stride=p.stride)
        if p.downsample is None:
            h = resnet.conv1x1(b, *p.conv3, skip=h)
        else:
            h = resnet.conv1x1(b, *p.conv3, skip=h, skip_params=p.downsample, skip_stride=p.stride)
        launches += 3
    assert launches == 18
    assert tuple(y.shape) == (TRUNK_M, TRUNK_COUT, 2, 2) and y.dtype == torch.bfloat16
    assert y.is_contiguous(memory_format=torch.channels_last)
    assert_same_bits(y.permute(0, 2, 3, 1), h)
    assert_same_bits(trunk(images.bfloat16()).permute(0, 2, 3, 1), h)    # bf16 images: the same rounding on the host


def test_stem_launch_against_the_torch_stem_on_the_cpu(device):
    """The stem launch against the stand-in's conv1, bn1, relu, maxpool on the CPU (float64, bf16 operands): within
    the contract's bar (stem_kit.check_bound).  The distance to the f32 modules is printed."""
    from mvn_rocm import resnet
    net_cpu = stand_in_backbone()
    case = cpu_stem(net_cpu, trunk_images())
    got = resnet.StemEval.from_reference(net_cpu, device=device)(trunk_images().to(device))
    check_bound(case, nchw(got).float(), "StemEval on the stand-in")
    with torch.no_grad():
        f32 = net_cpu.stem(trunk_images())
    err = float((nchw(got).float() - f32).abs().max()) / float(f32.abs().max())
    print(f"StemEval against the f32 modules on unrounded images: max error / max|ref| = {err:.3e}")   # a figure, not a bar


def test_backbone_eval_with_the_kernel_stem(device):
    """BackboneEval(trunk="kernels", stem="kernels") returns the 4-tuple with the shapes and dtypes of the default."""
    from mvn_rocm import backbone, resnet
    net, images = on_device(device)
    bt = backbone.BackboneEval.from_reference(net, device=device, feature_dtype=torch.float32)
    bk = backbone.BackboneEval.from_reference(net, device=device, feature_dtype=torch.float32, trunk="kernels", stem="kernels")
    assert isinstance(bk.trunk.stem, resnet.StemEval)
    with torch.no_grad():
        want, got = bt(images), bk(images)
        x4 = bk.trunk(images)
        hm_w, f_w = bk.head(x4)
        vc_w = net.vol_confidences(x4.float())
    assert len(got) == len(want) == 4
    for g, w in zip(got, want):
        assert tuple(g.shape) == tuple(w.shape) and g.dtype == w.dtype
    assert_same_bits(got[0], hm_w)
    assert_same_bits(got[1], f_w)
    assert torch.equal(got[3], vc_w)
    err = float((got[1] - want[1]).abs().max()) / float(want[1].abs().max())
    print(f"features, kernel stem and trunk against torch f32: max error / max|ref| = {err:.3e}")   # a figure, not a bar


def test_volumetric_model_with_the_kernel_stem(device):
    """VolumetricModelEval(trunk="kernels", stem="kernels") at B = 1, N = 3, V = 32 equals VolumetricEval fed the
    separately computed features, bit for bit."""
    from mvn_rocm import backbone, model, resnet, synth
    B, N, V = 1, 3, 32
    net = copy.deepcopy(stand_in_trunk_model()).to(device)
    images = trunk_images().to(device).view(B, N, 3, 40, 56)
    vb = synth.volumetric_batch(B, n_views=N, channels=8, heatmap=16, volume=V, seed=3)
    proj, coords = vb.proj.to(device), vb.cuboids(device)
    me = model.VolumetricModelEval.from_reference(net, device=device, fused=False, trunk="kernels", stem="kernels")
    assert isinstance(me.backbone.trunk.stem, resnet.StemEval)
    be = backbone.BackboneEval.from_reference(net.backbone, device=device, heatmaps=False, trunk="kernels", stem="kernels")
    ev = model.VolumetricEval.from_reference(net, device=device)
    with torch.no_grad():
        got = me(images, proj, coords)
        _, f, _, vc = be(images.view(B * N, 3, 40, 56))
        want = ev(f.view(B, N, *f.shape[1:]), proj, coords, vc.view(B, N, 32))
    assert tuple(got[0].shape) == (B, 5, 3) and bool(torch.isfinite(got[0]).all())
    assert tuple(got[1].shape) == (B, N, 32, 16, 16)
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if g is not None:
            assert_same_bits(g, w)


def test_the_traced_op_runs(device):
    """torch.ops.mvn_rocm.stem through the dispatcher, and a make_fx graph of it replayed on the device."""
    from torch.fx.experimental.proxy_tensor import make_fx
    from mvn_rocm import resnet
    net, images = on_device(device)
    p = resnet.fold_stem(net.conv1, net.bn1, net.relu, net.maxpool, device=device)
    want = resnet.stem(images, *p)
    assert_same_bits(torch.ops.mvn_rocm.stem(images, *p), want)
    gm = make_fx(lambda x, pk, sc, sh: resnet.stem(x, pk, sc, sh), tracing_mode="fake")(images, *p)
    assert [n.target for n in gm.graph.nodes if n.op == "call_function"].count(torch.ops.mvn_rocm.stem.default) == 1
    assert_same_bits(gm(images, *p), want)
