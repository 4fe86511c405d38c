"""What the tests of the confidence heads' kernels share (tests/test_confidence_api.py, test_gpu_conv3x3_pool.py,
test_gpu_confidence_tail.py, test_gpu_confidence_head_eval.py, test_gpu_algebraic_model_eval.py): the operands
of one mvn_conv3x3_pool / mvn_confidence_tail launch on the CPU, the contracts of include/mvn_hip.h restated
with F.conv2d / F.max_pool2d (f32 where the sums are exact, float64 otherwise) and with the exact f32 fma of
tests/test_feature_conv_api.py, the contracts' error bounds, index weights, the unpackers by the documented
layouts, and the stand-in GlobalAveragePoolingHead, backbone and models, written from torch.nn under the
reference's attribute names.  Nothing here is read from the code under test.  Not a test module and not a
conftest.  Reads nothing outside the repository.

The pool kernel's tiles, restated: it runs over the flat pool windows q = (n, py, px) of the whole batch; an
MFMA fragment is 16 consecutive windows (one of their four conv pixels each); a block is one 16-window tile of 64
output channels; a K-step is 32 input channels of one tap, steps tap-major, two per loop pass, and the block's four
waves take the K-steps [s per, (s + 1) per), per = ceil(9 Cin / 32 / 4) rounded up to even (Cin = 64: 6, 6, 6 and
none; 192: 14, 14, 14, 12, inside a tap; 512: 36 each; 2048: 144 each).  So the seams are at flat windows 16 k, at
output channels 64 k and at those K-steps.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from bottleneck_kit import index_weight1, make_layer
from deconv_kit import cl2d, randomise2d
from test_feature_conv_api import fma32
from v2v_kit import bf16r, exact_scale_shift, unpack_mfma_a

TILE_WIN, BLOCK_WIN, GROUP_C = 16, 64, 64

# (M, Cin, H, W, Cout)
POOL_SHAPES = (
    (1, 64, 2, 2, 64),          # one window; five of nine taps are padding somewhere
    (2, 64, 3, 3, 64),          # odd sizes: the dropped row and column are still read as taps
    (1, 64, 5, 7, 128),         # odd both ways, two channel groups
    (3, 64, 4, 6, 64),          # 18 windows: three images inside one tile, and the seam after 16 windows
    (1, 192, 4, 4, 64),         # 6 K-steps per tap, not a power of two; K slices of 14, 14, 14, 12
    (1, 64, 18, 20, 64),        # 90 windows: five tiles and a ragged sixth
    (1, 512, 6, 6, 256),        # the real second layer, 3 x 3 out
    (1, 2048, 4, 4, 512),       # the real first layer, K = 18432, all 576 steps
)
SUBSET = ((2, 64, 3, 3, 64), (3, 64, 4, 6, 64), (1, 64, 18, 20, 64), (1, 192, 4, 4, 64))

# (M, h w, C0, C1, C2, n)
TAIL_SHAPES = ((1, 1, 64, 64, 64, 1), (5, 6, 64, 128, 64, 5), (2, 4, 256, 512, 256, 32), (3, 9, 256, 512, 256, 17))


def shape_id(s):
    return "x".join(map(str, s))


def per_channel(t):
    return t.double().view(1, -1, 1, 1)


def relu64(r):
    return torch.where(r <= 0, torch.zeros_like(r), r)               # a NaN is neither: kept


def conv3(x, w):
    return F.conv2d(x, w, None, stride=1, padding=1)


def pool(r):
    """MaxPool2d(2), floor mode: a NaN in a window gives NaN."""
    return F.max_pool2d(r, 2)


def _finite(t):
    return torch.where(torch.isfinite(t), t, torch.zeros_like(t))


def nchw(y_cl):
    return y_cl.cpu().permute(0, 3, 1, 2).contiguous()


class PoolCase:
    """Operands of one mvn_conv3x3_pool launch on the CPU: x (M, Cin, H, W), w (Cout, Cin, 3, 3), scale, shift
    (Cout,) f32 tensors of bf16-exact values."""

    def __init__(self, x, w, scale, shift):
        assert w.shape[1] == x.shape[1] and tuple(w.shape[2:]) == (3, 3) and scale.shape == shift.shape == (w.shape[0],)
        self.x, self.w, self.scale, self.shift = x, w, scale, shift

    @property
    def gamma(self):
        """9 Cin products and the fma."""
        return (9 * self.x.shape[1] + 1) * 2.0 ** -24

    def run(self, device, out_dtype=torch.bfloat16, x_dev=None):
        from mvn_rocm import confidence
        assert bool((self.w.bfloat16().float() == self.w).all())
        xd = cl2d(self.x, device) if x_dev is None else x_dev
        return confidence.conv3x3_pool(xd, confidence.pack_conv3x3_pool_weight(self.w.double()).to(device),
                                       self.scale.to(device), self.shift.to(device), out_dtype=out_dtype)

    def abs_terms(self):
        """S per conv pixel, float64, non-finite values left out."""
        return conv3(_finite(self.x).double().abs(), self.w.double().abs()) * per_channel(self.scale).abs() + per_channel(self.shift).abs()

    def pre_pool(self, f32=True):
        """r_q of the contract per conv pixel in float64, the convolution in f32 on the CPU (``f32``) or in float64."""
        acc = conv3(self.x, self.w).double() if f32 else conv3(self.x.double(), self.w.double())
        return acc * per_channel(self.scale) + per_channel(self.shift)

    def reference(self):
        """The f32 reference (M, Cout, H // 2, W // 2) for operands on which no order of accumulation rounds: the
        sums of |x w| stay below 2^24 and fma(acc, scale, shift) is exact in f32 (both asserted)."""
        assert float(conv3(_finite(self.x).abs(), self.w.abs()).max()) < 2.0 ** 24
        r = self.pre_pool()
        assert bool(((r.float().double() == r) | torch.isnan(r)).all()), "fma(acc, scale, shift) is not exact in f32"
        assert not bool((torch.signbit(r) & (r == 0)).any()), "the pre-pool reference holds a -0"
        return relu64(pool(r)).float()


def _ints(g, *shape):
    return torch.randint(-4, 5, shape, generator=g).float()


def integer_pool(shape, seed):
    """Integers in [-4, 4], scale +-2^k of both signs, shift in quarters: every sum is exact in f32 in any order."""
    M, cin, H, W, cout = shape
    g = torch.Generator().manual_seed(seed)
    return PoolCase(_ints(g, M, cin, H, W), _ints(g, cout, cin, 3, 3), *exact_scale_shift(seed + 1, cout))


def _seed(shape):
    return sum((7 * i + 3) * v for i, v in enumerate(shape))


@functools.lru_cache(maxsize=None)
def parity_pool(shape):
    """The integer case of a shape and its reference, computed once and shared (read-only)."""
    case = integer_pool(shape, _seed(shape))
    return case, case.reference()


def random_pool(shape, seed):
    """randn inputs, weights of std 3 sqrt(2 / (9 (Cin + Cout))), scale in [0.75, 1.25] of both signs; bf16-exact."""
    M, cin, H, W, cout = shape
    g = torch.Generator().manual_seed(seed)
    x = bf16r(torch.randn(M, cin, H, W, generator=g))
    w = bf16r(torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * (cin + cout))) ** 0.5 * 3)
    scale = (0.75 + 0.5 * torch.rand(cout, generator=g)) * torch.where(torch.arange(cout) % 5 == 2, -1.0, 1.0)
    return PoolCase(x, w, scale, 0.2 * torch.randn(cout, generator=g))


def pool_bound(case):
    """(ref, the f32 term of the bar, the worst fraction of gamma S at which the f32 CPU convolution sits):
    ref = relu(max over the window of r_q) in float64; the bar carries gamma S through the maximum (|max a -
    max b| <= max |a - b|, and the ReLU does not expand), gamma = (9 Cin + 1) 2^-24."""
    gS = case.gamma * case.abs_terms()
    r = case.pre_pool(f32=False)
    cpu_frac = float(((case.pre_pool(f32=True) - r).abs() / gS).max())
    return relu64(pool(r)), pool(gS), cpu_frac


def check_pool_bound(case, got, what, f32_out):
    """|got - ref| <= 2^-8 |ref| + max over the window's four pixels of gamma S per element, without the first
    term for an f32 output: bottleneck_kit.check_bound's bar carried through the maximum, with its guard that
    the f32 CPU convolution sits within 0.05 of gamma S (a bound for these inputs, no measurement)."""
    ref, bar32, cpu_frac = pool_bound(case)
    bar = bar32 if f32_out else 2.0 ** -8 * ref.abs() + bar32
    frac = float(((got.double() - ref).abs() / bar).max())
    print(f"{what}: worst |got - ref| / bar = {frac:.4f}; the f32 CPU convolution at {cpu_frac:.4f} of gamma S")
    assert cpu_frac <= 0.05, "the f32 CPU convolution is not far inside gamma S: the bar is no bound for these inputs"
    assert frac <= 1.0
    return frac


# ----------------------------------------------------------------------------- index weights, unpackers
def index_weight_pool(cout, cin):
    """A bf16-exact (Cout, Cin, 3, 3) weight that encodes its own index: ``bottleneck_kit.index_weight1`` for
    (co, ci), the tap in the exponent."""
    tap = torch.arange(9).view(1, 1, 3, 3)
    w = (index_weight1(cout, cin).double().view(cout, cin, 1, 1) * torch.exp2((16 * tap - 32).double())).float().contiguous()
    assert bool((w.bfloat16().float() == w).all()) and bool(torch.isfinite(w).all()) and bool((w != 0).all())
    return w


def unpack_pool(packed, cout, cin):
    """The (Cout, Cin, 3, 3) weight from the documented layout (include/mvn_hip.h):
    [tap = ky*3 + kx][kp][m][lane][j] = w[16 m + (lane & 15)][32 kp + 8 (lane >> 4) + j][ky][kx]."""
    assert tuple(packed.shape) == (9, cin // 32, cout // 16, 64, 8) and packed.dtype == torch.bfloat16
    a = unpack_mfma_a(packed)                                    # (9, KP, cout rows, 32 K-slots)
    return a.permute(2, 1, 3, 0).reshape(cout, cin, 3, 3)


def element_pool(packed, tap, kp, m, lane, j):
    """The documented element formula read literally: ((co, ci, ky, kx), value)."""
    return (16 * m + (lane & 15), 32 * kp + 8 * (lane >> 4) + j, tap // 3, tap % 3), float(packed[tap, kp, m, lane, j])


# ----------------------------------------------------------------------------- the tail
def tail_offsets(c0, c1, c2, n):
    """O1 .. O5 and the size of the packed parameters (include/mvn_hip.h)."""
    o1 = c0 * c1
    o2 = o1 + c1
    o3 = o2 + c1 * c2
    o4 = o3 + c2
    o5 = o4 + c2 * n
    return o1, o2, o3, o4, o5, o5 + n


def unpack_tail(packed, widths):
    """[(W1, b1), (W2, b2), (W3, b3)] with W (out, in) from the documented layout: params[O + i * out + o] = W[o][i]."""
    c0, c1, c2, n = widths
    o1, o2, o3, o4, o5, size = tail_offsets(*widths)
    p = packed.cpu()
    assert p.dtype == torch.float32 and tuple(p.shape) == (size,)
    return [(p[0:o1].view(c0, c1).t(), p[o1:o2]), (p[o2:o3].view(c1, c2).t(), p[o3:o4]), (p[o4:o5].view(c2, n).t(), p[o5:size])]


def tail_element(packed, widths, layer, i, o):
    """The documented element formula read literally: the packed word that holds W_layer[o][i] (layer 1..3)."""
    c0, c1, c2, n = widths
    o1, o2, o3, o4, o5, _ = tail_offsets(*widths)
    base, out = ((0, c1), (o2, c2), (o4, n))[layer - 1]
    return float(packed[base + i * out + o])


def tail_logits(pooled, linears):
    """mvn_confidence_tail's contract with MVN_ACT_NONE restated in numpy f32: pooled (M, hw, C0), linears three
    (W (out, in), b) pairs -> (M, n).  The mean adds the pixels in ascending order from +0 and divides once; each
    Linear is acc = b[o], then acc = fma32(W[o][i], x[i], acc) for i ascending; the ReLU keeps a NaN."""
    x = np.asarray(pooled, np.float32)
    s = np.zeros((x.shape[0], x.shape[2]), np.float32)
    for p in range(x.shape[1]):
        s = (s + x[:, p, :]).astype(np.float32)
    v = (s / np.float32(x.shape[1])).astype(np.float32)
    for k, (W, b) in enumerate(linears):
        W, b = np.asarray(W, np.float32), np.asarray(b, np.float32)
        acc = np.broadcast_to(b[None, :], (v.shape[0], W.shape[0])).astype(np.float32)
        for i in range(W.shape[1]):
            acc = fma32(W[None, :, i], v[:, i, None], acc)
        v = np.where(acc <= 0, np.float32(0.0), acc).astype(np.float32) if k < 2 else acc
    return v


def random_tail(shape, seed, integers=False):
    """(pooled (M, hw, C0) f32, linears) for a tail shape: non-negative maps as behind a ReLU; ``integers``: small
    integer maps whose pixel count divides their sum, integer weights and biases (every chain exact in f32)."""
    M, hw, c0, c1, c2, n = shape
    g = torch.Generator().manual_seed(seed)
    if integers:
        pooled = torch.randint(0, 3, (M, 1, c0), generator=g).float().expand(M, hw, c0).contiguous()
        mk = lambda o, i: (torch.randint(-1, 2, (o, i), generator=g).float(), torch.randint(-3, 4, (o,), generator=g).float())
    else:
        pooled = torch.randn(M, hw, c0, generator=g).abs()
        mk = lambda o, i: (torch.randn(o, i, generator=g) * (2.0 / i) ** 0.5, torch.randn(o, generator=g) * 0.1)
    return pooled, [mk(c1, c0), mk(c2, c1), mk(n, c2)]


# ----------------------------------------------------------------------------- stand-in modules
class GlobalAveragePoolingHead(nn.Module):
    """The reference's head by attribute names and forward order: two (3x3 convolution with bias, BatchNorm,
    MaxPool2d(2), ReLU) stages, the mean over the pixels, three Linear layers with ReLUs and a Sigmoid; the
    widths are arguments (the reference's are 512, 256 and 512, 256)."""

    def __init__(self, in_channels, n_classes, c1=512, c2=256, l1=512, l2=256):
        super().__init__()
        self.features = nn.Sequential(
            nn.Conv2d(in_channels, c1, 3, stride=1, padding=1), nn.BatchNorm2d(c1), nn.MaxPool2d(2), nn.ReLU(inplace=True),
            nn.Conv2d(c1, c2, 3, stride=1, padding=1), nn.BatchNorm2d(c2), nn.MaxPool2d(2), nn.ReLU(inplace=True))
        self.head = nn.Sequential(nn.Linear(c2, l1), nn.ReLU(inplace=True), nn.Linear(l1, l2), nn.ReLU(inplace=True),
                                  nn.Linear(l2, n_classes), nn.Sigmoid())

    def forward(self, x):
        x = self.features(x)
        batch_size, n_channels = x.shape[:2]
        x = x.view((batch_size, n_channels, -1)).mean(dim=-1)
        return self.head(x)


def randomise_head(head, seed):
    """Xavier-like weights, small biases and BatchNorm statistics of a trained layer's order of magnitude; eval."""
    randomise2d(head, seed, bias=0.05)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in head.modules():
            if isinstance(m, nn.Linear):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / m.in_features) ** 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
    return head.eval()


@functools.lru_cache(maxsize=None)
def small_head():
    """64 -> 64 -> 64 convolutions, tail 64-128-64-5 (read-only: copy before moving it)."""
    return randomise_head(GlobalAveragePoolingHead(64, 5, 64, 64, 128, 64), seed=61)


@functools.lru_cache(maxsize=None)
def real_head():
    """The reference's widths behind 2048 channels, n = 17."""
    return randomise_head(GlobalAveragePoolingHead(2048, 17), seed=63)


def head_reference(head, x):
    """The head on the CPU as the three launches compute it, in float64 with the convolutions' operands rounded
    to bf16 and the first stage's output rounded to bf16: x (M, Cin, h, w) bf16-exact f32.  Returns (the float64
    confidences, the bound per element), in the manner of ``bottleneck_kit.block_reference``: per convolution
    gamma S through the maximum, one bf16 ulp (2^-7 |value|) where a stage rounds, carried through what follows
    by the absolute weights; (count + 1) u S for the mean and each Linear; the sigmoid has slope at most 1 / 4
    and adds 4 u."""
    u = 2.0 ** -24
    feats, lin = head.features, head.head

    def fold(conv, bn):
        s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
        t = (conv.bias.double() - bn.running_mean.double()) * s + bn.bias.double()
        return bf16r(conv.weight.detach()).double(), s.float().double(), t.float().double()

    def stage(h, err, conv, bn):
        w, s, t = fold(conv, bn)
        n = w[0].numel()
        r = conv3(h, w) * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1)
        S = conv3(h.abs(), w.abs()) * s.abs().view(1, -1, 1, 1) + t.abs().view(1, -1, 1, 1)
        c = conv3(err, w.abs()) * s.abs().view(1, -1, 1, 1)
        return relu64(pool(r)), pool(c + (n + 1) * u * (S + c))

    with torch.no_grad():
        x64 = x.double()
        y1, e1 = stage(x64, torch.zeros_like(x64), feats[0], feats[1])
        h1 = bf16r(y1).double()
        e1 = e1 + 2.0 ** -7 * h1.abs() + 2.0 ** -7 * e1               # the kernel rounds a value within e1 of y1
        y2, e2 = stage(h1, e1, feats[4], feats[5])
        hw = y2.shape[2] * y2.shape[3]
        v = y2.flatten(2).mean(-1)
        e = e2.flatten(2).mean(-1)
        e = e + (hw + 1) * u * (v.abs() + e)
        for k in (0, 2, 4):
            W, b = lin[k].weight.double(), lin[k].bias.double()
            S = v.abs() @ W.abs().t() + b.abs()
            c = e @ W.abs().t()
            v = v @ W.t() + b
            e = c + (W.shape[1] + 1) * u * (S + c)
            if k < 4:
                v = relu64(v)
        return torch.sigmoid(v), e / 4 + 4 * u


def head_stage_bounds(head, x, h1, h2):
    """The head launch by launch, each against its own contract in float64 on the input it really read: x
    (M, Cin, h, w) bf16-exact f32; h1 (M, C1, h/2, w/2) the first launch's bf16 output and h2 (M, C2, h/4, w/4) the
    second's f32 output as NCHW tensors on the CPU.  Returns [(name, reference, bound), ...] for h1 (from x:
    2^-8 |ref| + max over the window of gamma S), h2 (from h1: max over the window of gamma S) and the confidences
    (from h2: (count + 1) u S for the mean and each Linear, carried through the Linears behind it by their absolute
    weights; the sigmoid has slope at most 1 / 4 and adds 4 u).  No bf16 rounding is carried across a launch, so
    every bound is a few f32 ulps of the sums it covers."""
    u = 2.0 ** -24
    feats, lin = head.features, head.head

    def stage(h, conv, bn):
        s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
        t = ((conv.bias.double() - bn.running_mean.double()) * s + bn.bias.double()).float().double()
        s, w = s.float().double(), bf16r(conv.weight.detach()).double()
        r = conv3(h, w) * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1)
        S = conv3(h.abs(), w.abs()) * s.abs().view(1, -1, 1, 1) + t.abs().view(1, -1, 1, 1)
        return relu64(pool(r)), pool((w[0].numel() + 1) * u * S)

    with torch.no_grad():
        y1, g1 = stage(x.double(), feats[0], feats[1])
        y2, g2 = stage(h1.double(), feats[4], feats[5])
        hw = h2.shape[2] * h2.shape[3]
        v = h2.double().flatten(2).mean(-1)
        e = (hw + 1) * u * v.abs()
        for k in (0, 2, 4):
            W, b = lin[k].weight.double(), lin[k].bias.double()
            S, c = v.abs() @ W.abs().t() + b.abs(), e @ W.abs().t()
            v = v @ W.t() + b
            e = c + (W.shape[1] + 1) * u * (S + c)
            if k < 4:
                v = relu64(v)
        return [("stage 1", y1, 2.0 ** -8 * y1.abs() + g1), ("stage 2", y2, g2), ("confidences", torch.sigmoid(v), e / 4 + 4 * u)]


MAPS_STRIDE = 8                                # images -> layer4's maps of StandInConfidenceBackbone
IMAGE = (64, 96)                                  # maps of 8 x 12, pooled to 4 x 6 and 2 x 3 by the heads
TRUNK_COUT = 256


class StandInConfidenceBackbone(nn.Module):
    """The reference's PoseResNet by attribute names and forward order: its stem, four stages of Bottleneck
    (strides 1, 2, 1, 1, so that 64 x 96 images leave 8 x 12 maps for the heads' two pools; 64-channel middles,
    256 channels out), three deconv triples, final_layer, and both confidence heads in the reference's form and
    widths (``with_alg=False``: no alg_confidences, the reference's backbone without use_confidences)."""

    def __init__(self, joints=17, with_alg=True):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = make_layer(64, 64, 2, 1)
        self.layer2 = make_layer(256, 64, 1, 2)
        self.layer3 = make_layer(256, 64, 1, 1)
        self.layer4 = make_layer(256, 64, 1, 1)
        if with_alg:
            self.alg_confidences = GlobalAveragePoolingHead(TRUNK_COUT, joints)
        self.vol_confidences = GlobalAveragePoolingHead(TRUNK_COUT, 32)
        layers, cin = [], TRUNK_COUT
        for _ in range(3):
            layers += [nn.ConvTranspose2d(cin, 256, 4, stride=2, padding=1, output_padding=0, bias=False),
                       nn.BatchNorm2d(256), nn.ReLU(inplace=True)]
            cin = 256
        self.deconv_layers = nn.Sequential(*layers)
        self.final_layer = nn.Conv2d(256, joints, 1)


def _randomise_backbone(net, seed):
    randomise2d(net, seed=seed, bias=0.02)
    for k, name in enumerate(("alg_confidences", "vol_confidences")):
        if hasattr(net, name):
            randomise_head(getattr(net, name), seed + 10 + k)
    return net.eval()


@functools.lru_cache(maxsize=None)
def stand_in_backbone(joints=17, with_alg=True):
    """The randomised stand-in on the CPU, built once (read-only: copy before moving it)."""
    return _randomise_backbone(StandInConfidenceBackbone(joints, with_alg), seed=71)


class StandInAlgebraicModel(nn.Module):
    """The attributes of AlgebraicTriangulationNet that AlgebraicModelEval reads."""

    def __init__(self, backbone, use_confidences, heatmap_softmax, heatmap_multiplier):
        super().__init__()
        self.backbone = backbone
        self.use_confidences = use_confidences
        self.heatmap_softmax = heatmap_softmax
        self.heatmap_multiplier = heatmap_multiplier


class StandInVolumetricModel(nn.Module):
    """The attributes of VolumetricTriangulationNet that VolumetricModelEval reads, with 'conf' aggregation."""

    def __init__(self, backbone, joints, multiplier):
        super().__init__()
        from v2v_kit import V2VModel
        self.backbone = backbone
        self.process_features = nn.Sequential(nn.Conv2d(256, 32, 1))
        self.volume_net = V2VModel(32, joints)
        self.volume_aggregation_method = "conf"
        self.volume_multiplier = multiplier
        self.volume_softmax = True


@functools.lru_cache(maxsize=None)
def stand_in_volumetric_model(joints=5, multiplier=10.0):
    from v2v_kit import randomise
    net = StandInVolumetricModel(_randomise_backbone(StandInConfidenceBackbone(joints), seed=71), joints, multiplier)
    randomise2d(net.process_features, seed=75, bias=0.1)
    randomise(net.volume_net, seed=2027)
    return net.eval()
