"""What the tests of mvn_deconv4s2_project share (tests/test_deconv_project_api.py,
test_gpu_deconv_project.py, test_gpu_volumetric_model_eval.py): the contract of include/mvn_hip.h
restated on the CPU (the hi | lo split in float64, the projection of an activation, the packed layout
read by its documented element formula) and the stand-in backbone and volumetric model of the
module tests.  Nothing here is read from the code under test.  Not a test module and not a conftest.
Reads nothing outside the repository.
"""
import functools

import torch
from torch import nn

from deconv_kit import COUT, randomise2d
from v2v_kit import V2VModel, randomise

ROWS = 32                                    # output channels of the projection
PACKED_SHAPE = (2, COUT // 32, ROWS // 16, 64, 8)
GAMMA = (2 * COUT + 4) * 2.0 ** -24          # 512 products, the bias and the final rounding (DESIGN.md §4.16's form)


def split(w):
    """(hi, lo) of the contract as float64 tensors: hi = bf16(w), lo = bf16(w - hi), for a float32 w."""
    assert w.dtype == torch.float32
    hi = w.bfloat16().double()
    d = w.double() - hi
    lo = d.float().bfloat16().double()
    assert bool((d.float().double() == d).all())                 # the difference is exact in f32: one rounding
    return hi, lo


def unpack_projection(packed):
    """(hi, lo) (32, 256) float64 from the documented layout (include/mvn_hip.h):
    [part][k][nt][lane][j] = part(w[16 nt + (lane & 15)][32 k + 16 (j >> 2) + 4 (lane >> 4) + (j & 3)])."""
    assert tuple(packed.shape) == PACKED_SHAPE and packed.dtype == torch.bfloat16
    part, k, nt, lane, j = torch.meshgrid(*(torch.arange(n) for n in PACKED_SHAPE), indexing="ij")
    row = 16 * nt + (lane & 15)
    col = 32 * k + 16 * (j >> 2) + 4 * (lane >> 4) + (j & 3)
    out = torch.full((2, ROWS, COUT), float("nan"), dtype=torch.float64)
    out[part, row, col] = packed.cpu().double()
    assert not bool(torch.isnan(out).any())                      # the formula reaches every (part, row, column) slot
    return out[0], out[1]


def project64(a, hi, lo, bias):
    """bias + sum_c a[c] (hi + lo)[p, c] in float64: a (M, 256, H, W) -> (M, 32, H, W)."""
    return torch.einsum("pc,mchw->mphw", hi + lo, a.double()) + bias.double().view(1, -1, 1, 1)


def abs_sum(a, hi, lo, bias):
    """S of the bound: |bias| + sum_c |a[c]| (|hi| + |lo|)."""
    return torch.einsum("pc,mchw->mphw", hi.abs() + lo.abs(), a.double().abs()) + bias.double().abs().view(1, -1, 1, 1)


def integer_projection(seed):
    """Integer weights in [-4, 4] (bf16-exact: lo = 0) and an integer bias in [-8, 8]."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randint(-4, 5, (ROWS, COUT), generator=g).float()
    b = torch.randint(-8, 9, (ROWS,), generator=g).float()
    assert bool((w.bfloat16().float() == w).all())
    return w, b


def exact_projection(ref, w, b, q=0.25):
    """The CPU value ``b + sum bf16(ref) w`` for data on which no order of accumulation rounds: every
    term is a multiple of the quantum q and |b| + sum |a w| stays below 2^24 q (both asserted).
    Returns (the f32 result, the bf16 activation as f32)."""
    a = ref.bfloat16().float()
    fin = torch.where(torch.isfinite(a), a, torch.zeros_like(a)).double()
    whole = lambda t: bool((t.double() == t.double().round()).all())
    assert whole(fin / q) and whole(w) and whole(b), "a term is no multiple of the quantum"
    S = torch.einsum("pc,mchw->mphw", w.double().abs(), fin.abs()) + b.double().abs().view(1, -1, 1, 1)
    assert float(S.max()) < 2.0 ** 24 * q, f"sum of the absolute terms {float(S.max())} is not below 2^24 q"
    out = torch.einsum("pc,mchw->mphw", w.double(), a.double()) + b.double().view(1, -1, 1, 1)
    out32 = out.float()
    assert bool(((out32.double() == out) | torch.isnan(out)).all())
    return out32, a


def index_projection():
    """A positive (32, 256) f32 weight that encodes its own (p, c) index in a full 16-bit significand,
    1 + (4 (256 p + c) + 1) 2^-15, so that lo != 0 everywhere and hi + lo == w exactly."""
    idx = torch.arange(ROWS).view(-1, 1) * COUT + torch.arange(COUT).view(1, -1)
    w = (1.0 + (4 * idx + 1).double() * 2.0 ** -15).float()
    hi, lo = split(w)
    assert bool((lo != 0).all()) and bool((hi + lo == w.double()).all()) and w.unique().numel() == ROWS * COUT
    return w


# ----------------------------------------------------------------------------- stand-in modules
M, CIN, H4, W4, J = 6, 64, 3, 4, 17


class ConfidenceHead(nn.Module):
    """The shape of the reference's GlobalAveragePoolingHead: maps -> (M, 32) in (0, 1)."""

    def __init__(self, cin, n):
        super().__init__()
        self.head = nn.Sequential(nn.Linear(cin, n), nn.Sigmoid())

    def forward(self, x):
        return self.head(x.mean(dim=(2, 3)))


class StandInBackbone(nn.Module):
    """The reference's PoseResNet by attribute names and forward order, at toy widths: a two-conv
    strided trunk from (M, 3, 12, 16) images to (M, 64, 3, 4), three deconv triples, final_layer."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 16, 3, stride=2, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(16)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.Identity()
        self.layer1, self.layer2, self.layer3 = nn.Identity(), nn.Identity(), nn.Identity()
        self.layer4 = nn.Sequential(nn.Conv2d(16, CIN, 3, stride=2, padding=1, bias=False), nn.BatchNorm2d(CIN), nn.ReLU(True))
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


class StandInModel(nn.Module):
    """The attributes of VolumetricTriangulationNet that VolumetricModelEval reads."""

    def __init__(self, joints, multiplier):
        super().__init__()
        self.backbone = StandInBackbone()
        self.process_features = nn.Sequential(nn.Conv2d(COUT, ROWS, 1))
        self.volume_net = V2VModel(32, joints)
        self.volume_aggregation_method = "softmax"
        self.volume_multiplier = multiplier
        self.volume_softmax = True


@functools.lru_cache(maxsize=None)
def stand_in_model(joints=5, multiplier=10.0):
    """The randomised stand-in on the CPU, built once (read-only: copy before moving it)."""
    net = StandInModel(joints, multiplier)
    randomise2d(net.backbone, seed=31, bias=0.02)
    randomise2d(net.process_features, seed=41, bias=0.1)
    randomise(net.volume_net, seed=2025)
    g = torch.Generator().manual_seed(32)
    with torch.no_grad():
        lin = net.backbone.vol_confidences.head[0]
        lin.weight.copy_(torch.randn(lin.weight.shape, generator=g) * 0.1)
        lin.bias.copy_(torch.randn(lin.bias.shape, generator=g) * 0.1)
    return net.eval()
