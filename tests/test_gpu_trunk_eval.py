"""``resnet.TrunkEval``, ``BackboneEval(trunk="kernels")`` and ``VolumetricModelEval(trunk="kernels")`` on the GPU
(DESIGN.md §4.18), on the stand-in backbone of tests/bottleneck_kit.py: the reference's stem, four stages of
Bottleneck at strides 1, 2, 2, 2 (two of them of two blocks, so both kinds of residual occur), ending at 256
channels; M = 3 images of 3 x 40 x 56, so the maps are 10 x 14, 5 x 7, 3 x 4 and 2 x 2."""
import copy

import pytest
import torch

from bottleneck_kit import (TRUNK_COUT, TRUNK_M, block_reference, stand_in_backbone, stand_in_trunk_model, trunk_images)
from deconv_kit import nchw
from v2v_kit import assert_same_bits, bf16r

pytestmark = pytest.mark.gpu


def on_device(device):
    return copy.deepcopy(stand_in_backbone()).to(device), trunk_images().to(device)


def test_forward_is_the_stem_the_cast_and_the_launches(device):
    """TrunkEval.forward equals the backbone's stem, one cast-and-permute and the three launches of every block
    made one by one, bit for bit; its output is a channels_last view that DeconvHeadEval reads without a copy."""
    from mvn_rocm import resnet
    net, images = on_device(device)
    trunk = resnet.TrunkEval.from_reference(net, device=device)
    assert trunk.stem[0] is net.conv1 and trunk.stem[3] is net.maxpool      # the backbone's own modules
    assert len(trunk.blocks) == 6
    with torch.no_grad():
        y = trunk(images)
        h = net.stem(images).permute(0, 2, 3, 1).to(torch.bfloat16).contiguous()
        shapes = []
        for block in net.blocks():
            p = resnet.fold_bottleneck(block, device=device)
            a = resnet.conv1x1(h, *p.conv1)
            b = resnet.conv3x3(a, *p.conv2, stride=p.stride)
            if p.downsample is None:
                h = resnet.conv1x1(b, *p.conv3, skip=h)
            else:
                h = resnet.conv1x1(b, *p.conv3, skip=h, skip_params=p.downsample, skip_stride=p.stride)
            shapes.append(tuple(h.shape[1:3]))
    assert shapes == [(10, 14), (10, 14), (5, 7), (3, 4), (3, 4), (2, 2)]
    assert tuple(y.shape) == (TRUNK_M, TRUNK_COUT, 2, 2) and y.dtype == torch.bfloat16
    assert y.is_contiguous(memory_format=torch.channels_last)
    assert_same_bits(y.permute(0, 2, 3, 1), h)
    # what DeconvHeadEval.forward makes of it: the same memory, no copy pass
    as_head = y.permute(0, 2, 3, 1)
    assert as_head.is_contiguous() and as_head.dtype == torch.bfloat16 and as_head.data_ptr() == y.data_ptr()
    with pytest.raises(RuntimeError, match="inference-only"):
        trunk(images)                                                 # the stem's parameters record a graph


def test_every_block_against_the_cpu_block(device):
    """Each block on the kernels against the stand-in's block on the CPU in float64 with every convolution's
    operands rounded to bf16 and the activations rounded to bf16 between the convolutions: within one bf16
    ulp + gamma S per convolution, carried through the convolutions behind it (bottleneck_kit.block_reference)."""
    from mvn_rocm import resnet
    net_cpu = stand_in_backbone()
    with torch.no_grad():
        x = bf16r(net_cpu.stem(trunk_images()))
        for i, block in enumerate(net_cpu.blocks()):
            ref, bar = block_reference(block, x)
            got = resnet.BottleneckCL.from_reference(block, device=device)(x.bfloat16().permute(0, 2, 3, 1).contiguous().to(device))
            frac = float(((nchw(got).double() - ref).abs() / bar).max())
            cpu = block(x).double()                                   # the f32 modules on the same bf16-exact input
            print(f"block {i}: worst |got - ref| / bar = {frac:.4f}; max |ref| {float(ref.abs().max()):.3f}, "
                  f"the f32 modules differ from ref by {float((cpu - ref).abs().max()):.3e}")
            assert frac <= 1.0
            x = nchw(got).float()                                     # the next block starts from the kernels' output


def test_backbone_eval_with_the_kernel_trunk(device):
    """BackboneEval(trunk="kernels") returns the 4-tuple with the shapes and dtypes of trunk="torch": the confidence
    heads stay f32 modules and get the trunk's output cast; the head reads the trunk's output itself."""
    from mvn_rocm import backbone, resnet
    net, images = on_device(device)
    bt = backbone.BackboneEval.from_reference(net, device=device, feature_dtype=torch.float32)
    bk = backbone.BackboneEval.from_reference(net, device=device, feature_dtype=torch.float32, trunk="kernels")
    assert isinstance(bk.trunk, resnet.TrunkEval) and not isinstance(bt.trunk, resnet.TrunkEval)
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
    # a figure, not a bar (the bar is test_trunk_against_the_f32_modules): the two trunks compute the same network
    err = float((got[1] - want[1]).abs().max()) / float(want[1].abs().max())
    print(f"features, kernels against torch f32 trunk: max error / max|ref| = {err:.3e}")


def test_volumetric_model_with_the_kernel_trunk(device):
    """VolumetricModelEval(trunk="kernels") at B = 1, N = 3, V = 32 equals VolumetricEval fed the separately computed
    features, bit for bit."""
    from mvn_rocm import backbone, model, synth
    B, N, V = 1, 3, 32
    net = copy.deepcopy(stand_in_trunk_model()).to(device)
    images = trunk_images().to(device).view(B, N, 3, 40, 56)
    vb = synth.volumetric_batch(B, n_views=N, channels=8, heatmap=16, volume=V, seed=3)
    proj, coords = vb.proj.to(device), vb.cuboids(device)
    me = model.VolumetricModelEval.from_reference(net, device=device, fused=False, trunk="kernels")
    be = backbone.BackboneEval.from_reference(net.backbone, device=device, heatmaps=False, trunk="kernels")
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


def test_trunk_against_the_f32_modules(device):
    """The true semantics: the stand-in's stem and stages in f32 on the CPU, against (a) TrunkEval and (b) the
    same modules run by torch on the GPU in bfloat16 channels_last.  Both round every convolution's operands
    and outputs to bf16; (a) is held to twice (b)'s error, max error over max |ref|, the bar of
    tests/test_gpu_backbone_eval.py.  Measured on the MI355X: DESIGN.md §4.18."""
    from mvn_rocm import resnet
    net_cpu = stand_in_backbone()
    net, images = on_device(device)
    with torch.no_grad():
        ref = net_cpu.trunk(trunk_images())
        a = resnet.TrunkEval.from_reference(net, device=device)(images)
        nb = copy.deepcopy(net).to(dtype=torch.bfloat16, memory_format=torch.channels_last)
        b = nb.trunk(images.to(torch.bfloat16).to(memory_format=torch.channels_last))

    def err(got):
        return float((got.float().cpu() - ref).abs().max()) / float(ref.abs().max())
    ea, eb = err(a), err(b)
    print(f"layer4's output against the f32 modules, max error / max|ref|: TrunkEval {ea:.3e}, torch in bfloat16 "
          f"channels_last {eb:.3e}")
    assert ea <= 2 * eb
