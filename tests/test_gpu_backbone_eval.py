"""backbone.DeconvHeadEval and backbone.BackboneEval on the GPU, on a stand-in
backbone built from torch.nn with the reference's attribute names (pose_resnet.py:184-318): a
two-conv strided "trunk" from (M, 3, 12, 16) images to (M, 64, 3, 4), ``deconv_layers`` of three
(ConvTranspose2d, BatchNorm2d, ReLU) triples 64 -> 256 -> 256 -> 256, ``final_layer`` to J = 17 and,
optionally, a tiny ``vol_confidences`` head; statistics randomised as v2v_kit.randomise does."""
import copy
import functools

import pytest
import torch
from torch import nn

from deconv_kit import COUT, deconv, per_channel, randomise2d
from v2v_kit import assert_same_bits, bf16r

pytestmark = pytest.mark.gpu

M, CIN, H4, W4, J = 6, 64, 3, 4, 17


class ConfidenceHead(nn.Module):
    """The shape of the reference's GlobalAveragePoolingHead: maps -> (M, 32) in (0, 1)."""

    def __init__(self, cin, n):
        super().__init__()
        self.head = nn.Sequential(nn.Linear(cin, n), nn.Sigmoid())

    def forward(self, x):
        return self.head(x.mean(dim=(2, 3)))


class StandInBackbone(nn.Module):
    """The reference's PoseResNet by attribute names and forward order, at toy widths."""

    def __init__(self, vol_confidences):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 16, 3, stride=2, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(16)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.Identity()
        self.layer1, self.layer2, self.layer3 = nn.Identity(), nn.Identity(), nn.Identity()
        self.layer4 = nn.Sequential(nn.Conv2d(16, CIN, 3, stride=2, padding=1, bias=False), nn.BatchNorm2d(CIN), nn.ReLU(True))
        if vol_confidences:
            self.vol_confidences = ConfidenceHead(CIN, 32)
        layers, cin = [], CIN
        for _ in range(3):
            layers += [nn.ConvTranspose2d(cin, COUT, 4, stride=2, padding=1, output_padding=0, bias=False),
                       nn.BatchNorm2d(COUT), nn.ReLU(inplace=True)]
            cin = COUT
        self.deconv_layers = nn.Sequential(*layers)
        self.final_layer = nn.Conv2d(COUT, J, 1)

    def trunk(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        return self.layer4(self.layer3(self.layer2(self.layer1(x))))

    def forward(self, x):
        x = self.trunk(x)
        vol = self.vol_confidences(x) if hasattr(self, "vol_confidences") else None
        features = self.deconv_layers(x)
        return self.final_layer(features), features, None, vol


@functools.lru_cache(maxsize=None)
def stand_in(vol_confidences=True):
    net = randomise2d(StandInBackbone(vol_confidences), seed=31, bias=0.02)
    if vol_confidences:
        with torch.no_grad():
            lin = net.vol_confidences.head[0]
            g = torch.Generator().manual_seed(32)
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=g) * 0.1)
            lin.bias.copy_(torch.randn(lin.bias.shape, generator=g) * 0.1)
    return net


@functools.lru_cache(maxsize=None)
def layer4_output():
    """(M, 64, 3, 4) f32: the stand-in trunk's own output on random images (non-negative, as a ReLU's)."""
    with torch.no_grad():
        return stand_in().trunk(torch.randn(M, 3, 12, 16, generator=torch.Generator().manual_seed(33)))


def final_padded(net, device):
    w, b = torch.zeros(32, COUT), torch.zeros(32)
    w[:J], b[:J] = net.final_layer.weight.detach().cpu().view(J, COUT), net.final_layer.bias.detach().cpu()
    return w.to(device), b.to(device)


def launches(net, x_dev, feature_dtype, device):
    """The head written out: the cast-and-permute, three deconv4s2 launches, feature_conv."""
    from mvn_rocm import backbone, model
    dl = net.deconv_layers
    p = [backbone.fold_deconv_block(dl[3 * i], dl[3 * i + 1], device=device) for i in range(3)]
    h0 = x_dev.permute(0, 2, 3, 1).to(torch.bfloat16).contiguous()
    h1 = backbone.deconv4s2(h0, p[0], "cl")
    h2 = backbone.deconv4s2(h1, p[1], "cl")
    f = backbone.deconv4s2(h2, p[2], "nchw", feature_dtype)
    hm = model.feature_conv(f, *final_padded(net, device), out_dtype=torch.float32)[:, :J].contiguous()
    return (h0, h1, h2, f), hm


# ----------------------------------------------------------------------------- launches
@pytest.mark.parametrize("fmt", ("f32", "f32_channels_last", "bf16_channels_last"))
@pytest.mark.parametrize("feature_dtype", (torch.bfloat16, torch.float32), ids=("bf16", "f32"))
def test_forward_is_the_launches(device, feature_dtype, fmt):
    from mvn_rocm import backbone
    net = stand_in()
    x = layer4_output().to(device)
    if fmt != "f32":
        x = x.to(memory_format=torch.channels_last)
    if fmt == "bf16_channels_last":
        x = x.to(torch.bfloat16)
    head = backbone.DeconvHeadEval.from_reference(net, device=device, feature_dtype=feature_dtype)
    with torch.no_grad():
        hm, f = head(x)
        (_, _, _, f_w), hm_w = launches(net, x, feature_dtype, device)
        head.heatmaps = False
        none, f2 = head(x)
    assert tuple(f.shape) == (M, COUT, 8 * H4, 8 * W4) and f.dtype == feature_dtype and f.is_contiguous()
    assert tuple(hm.shape) == (M, J, 8 * H4, 8 * W4) and hm.dtype == torch.float32 and hm.is_contiguous()
    assert_same_bits(f, f_w)
    assert_same_bits(hm, hm_w)
    assert none is None
    assert_same_bits(f2, f_w)


# ----------------------------------------------------------------------------- the bf16-operand model, per layer
def bf16_ulp(ref):
    """One unit in the last place of bf16 at |ref| (0 at 0)."""
    a = ref.abs()
    return torch.where(a > 0, torch.exp2(torch.floor(torch.log2(a.clamp_min(2.0 ** -120))) - 7), torch.zeros_like(a))


def test_each_layer_against_the_bf16_operand_model(device):
    """Layer by layer, on the kernel chain's own inputs: the stand-in's triple on the CPU with both
    deconv operands rounded to bf16, in float64.  The bar: one bf16 ulp of the reference (the output's
    rounding; the float64 BatchNorm and the folded f32 scale / shift differ within it) plus the
    deconv test's gamma S, gamma = (4 Cin + 4) 2^-24.  The same triple in f32 on the CPU must stay
    inside the bar."""
    net = stand_in()
    x = layer4_output()
    with torch.no_grad():
        (h0, h1, h2, f), _ = launches(net, x.to(device), torch.bfloat16, device)
        ins = [h0, h1, h2]
        outs = [h1.cpu().permute(0, 3, 1, 2), h2.cpu().permute(0, 3, 1, 2), f.cpu()]
        for i in range(3):
            d, bn = net.deconv_layers[3 * i], net.deconv_layers[3 * i + 1]
            xin = ins[i].cpu().permute(0, 3, 1, 2).float()                           # bf16-exact
            wb = bf16r(d.weight.detach())
            s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
            t = bn.bias.double() - bn.running_mean.double() * s
            r = deconv(xin.double(), wb.double()) * per_channel(s) + per_channel(t)
            ref = torch.where(r <= 0, torch.zeros_like(r), r)
            gamma = (4 * xin.shape[1] + 4) * 2.0 ** -24
            S = deconv(xin.double().abs(), wb.double().abs()) * per_channel(s).abs() + per_channel(t).abs()
            bar = bf16_ulp(ref) + gamma * S
            cpu = torch.relu(bn(deconv(xin, wb)))
            cpu_frac = float(((cpu.double() - ref).abs() / bar).max())
            frac = float(((outs[i].double() - ref).abs() / bar).max())
            print(f"layer {i}: worst |got - ref| / bar = {frac:.4f}; the f32 CPU triple at {cpu_frac:.4f}")
            assert cpu_frac <= 1.0, "the f32 CPU model is outside the bar: the bar is no bound for these inputs"
            assert frac <= 1.0


# ----------------------------------------------------------------------------- the unrounded f32 modules
def test_against_the_f32_modules(device):
    """The true semantics: the stand-in's deconv_layers and final_layer in f32 on the CPU, against
    (a) DeconvHeadEval and (b) the same modules run by torch on the GPU in bfloat16 channels_last.
    Both round every layer's operands and outputs to bf16; (a) is held to twice (b)'s error, the form
    of tests/test_gpu_volumetric_eval.py.  Measured on the MI355X: DESIGN.md §4.16."""
    from mvn_rocm import backbone
    net = stand_in()
    x = layer4_output()
    with torch.no_grad():
        f_ref = net.deconv_layers(x)
        hm_ref = net.final_layer(f_ref)
        head = backbone.DeconvHeadEval.from_reference(net, device=device)
        hm_a, f_a = head(x.to(device))
        nb = copy.deepcopy(nn.Sequential(net.deconv_layers, net.final_layer)).to(
            device=device, dtype=torch.bfloat16, memory_format=torch.channels_last)
        f_b = nb[0](x.to(device).to(torch.bfloat16).to(memory_format=torch.channels_last))
        hm_b = nb[1](f_b)

    def err(got, ref):
        return float((got.float().cpu() - ref).abs().max()) / float(ref.abs().max())
    fa, fb, ha, hb = err(f_a, f_ref), err(f_b, f_ref), err(hm_a, hm_ref), err(hm_b, hm_ref)
    print(f"DeconvHeadEval against the f32 modules: features {fa:.3e} of max|ref|, heatmaps {ha:.3e}; "
          f"torch in bfloat16: features {fb:.3e}, heatmaps {hb:.3e}")
    assert fa <= 2 * fb
    assert ha <= 2 * hb


# ----------------------------------------------------------------------------- BackboneEval
@pytest.mark.parametrize("vol", (True, False), ids=("vol_confidences", "no_heads"))
def test_backbone_eval_returns_the_references_tuple(device, vol):
    from mvn_rocm import backbone
    net = copy.deepcopy(stand_in(vol)).to(device)
    images = torch.randn(M, 3, 12, 16, generator=torch.Generator().manual_seed(34)).to(device)
    be = backbone.BackboneEval.from_reference(net, device=device, feature_dtype=torch.float32)
    assert be.trunk[0] is net.conv1 and be.trunk[7] is net.layer4               # the backbone's own modules
    with torch.no_grad():
        hm, f, alg, vc = be(images)
        x4 = net.trunk(images)
        hm_w, f_w = backbone.DeconvHeadEval.from_reference(net, device=device, feature_dtype=torch.float32)(x4)
        _, _, _, vc_w = net(images)
    assert alg is None and (vc is None) == (not vol)
    assert_same_bits(f, f_w)
    assert_same_bits(hm, hm_w)
    if vol:
        assert tuple(vc.shape) == (M, 32) and torch.equal(vc, vc_w)
    with pytest.raises(RuntimeError, match="inference-only"):
        be(images)                                                       # the trunk's parameters record a graph


# ----------------------------------------------------------------------------- BackboneEval -> VolumetricEval
def test_composition_with_volumetric_eval(device):
    """The composition of INTEGRATION.md on the tiny shapes of tests/test_gpu_volumetric_eval.py (B = 2,
    N = 3, V = 32): the joints equal VolumetricEval fed the separately computed features, bit for bit."""
    from mvn_rocm import backbone, model, synth
    from test_feature_conv_api import stand_in_net
    from v2v_kit import E2E_MULT
    B, N, V = 2, 3, 32
    assert B * N == M
    vb = synth.volumetric_batch(B, n_views=N, channels=8, heatmap=8 * H4, volume=V, seed=3)
    vol_net = stand_in_net(seed=2025, J=5, multiplier=E2E_MULT)
    net = copy.deepcopy(stand_in(True)).to(device)
    images = torch.randn(M, 3, 12, 16, generator=torch.Generator().manual_seed(35)).to(device)
    be = backbone.BackboneEval.from_reference(net, device=device, heatmaps=False)
    ev = model.VolumetricEval.from_reference(vol_net, device=device)
    proj, coords = vb.proj.to(device), vb.cuboids(device)
    with torch.no_grad():
        _, features, _, vc = be(images)
        kp, f32, _, _ = ev(features.view(B, N, *features.shape[1:]), proj, coords, vc.view(B, N, 32))
        x4 = net.trunk(images)
        (_, _, _, f_w), _ = launches(net, x4, torch.bfloat16, device)
        kp_w, f32_w, _, _ = ev(f_w.view(B, N, *f_w.shape[1:]), proj, coords)
    assert tuple(kp.shape) == (B, 5, 3) and bool(torch.isfinite(kp).all())
    assert_same_bits(features, f_w)
    assert_same_bits(f32, f32_w)
    assert_same_bits(kp, kp_w)
