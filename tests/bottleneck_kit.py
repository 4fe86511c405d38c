"""What the tests of the ResNet trunk's kernels share (tests/test_bottleneck_api.py, test_gpu_bottleneck.py,
test_gpu_trunk_eval.py): the operands of one mvn_conv1x1 / mvn_conv3x3 launch on the CPU, the arithmetic
contracts of include/mvn_hip.h restated with F.conv2d (f32 where the sums are exact, float64 otherwise),
the contracts' error bound, index weights, the unpackers by the documented layouts, and the stand-in
Bottleneck and backbone, written from torch.nn under the reference's attribute names.  Nothing here is
read from the code under test.  Not a test module and not a conftest.  Reads nothing outside the
repository.

The kernels' tiles, restated: both run over the flat output pixels p = (n, oy, ox) of the whole batch;
an MFMA fragment is 16 consecutive pixels, a wave takes 64, a block 256; a block takes 64 output
channels; a K-step is 32 input channels (of one tap), two steps per loop pass.  So the seams are at flat
pixels 16 k, 64 k and 256 k, wherever those fall in the images, and at output channels 64 k.
"""
import functools

import torch
import torch.nn.functional as F
from torch import nn

from deconv_kit import cl2d, nchw, randomise2d
from v2v_kit import IDENTITY, NONE, POINTWISE, bf16r, exact_scale_shift, unpack_mfma_a

FRAG_PIX, WAVE_PIX, BLOCK_PIX, GROUP_C = 16, 64, 256, 64

# (M, Cin, H, W, Cout)
CONV1_SHAPES = (
    (2, 64, 1, 1, 64),          # smallest
    (3, 64, 3, 5, 256),         # image boundaries inside a pixel tile, M H W = 45; four channel groups
    (1, 256, 9, 15, 64),        # 135 pixels: two full waves and a ragged third (7 pixels of its first fragment)
    (1, 2048, 2, 3, 512),       # longest K
    (1, 512, 4, 3, 2048),       # widest output
    (1, 64, 17, 17, 128),       # 289 pixels: across the 256-pixel block seam, one pixel into a fragment; two groups
)
# the pointwise skip: (x shape, Cs, stride, Hs, Ws)
POINTWISE_CASES = (
    ((3, 64, 3, 5, 256), 64, 1, 3, 5),        # stride 1, from a map of the same size
    ((3, 64, 3, 5, 256), 256, 2, 5, 9),       # stride 2, odd sizes: the last row and column are read
    ((2, 128, 3, 4, 512), 256, 2, 6, 8),      # stride 2, even sizes: they are not
    ((1, 64, 17, 17, 128), 64, 2, 33, 34),    # across the block seam
)
# (M, C, H, W, stride)
CONV3_SHAPES = (
    (2, 64, 1, 1, 1), (2, 64, 1, 1, 2),       # one pixel, every tap but the centre is padding
    (1, 64, 3, 5, 1),           # odd sizes, stride 1
    (1, 64, 5, 7, 2),           # odd sizes: the last output row and column read the bottom and right padding
    (1, 64, 6, 8, 2),           # even sizes: they do not
    (1, 128, 12, 12, 2),        # the real net's second width, strided; two channel groups
    (1, 512, 3, 4, 1),          # K = 4608
    (1, 64, 20, 18, 1),         # 360 pixels: more than one tile both ways (fragment, wave and block seams)
    (3, 64, 4, 5, 1),           # three images inside one wave tile: no tap may read the neighbouring image
    (2, 192, 5, 7, 2),          # 6 K-steps per tap (no power of two), two images in a fragment, three groups
)


def shape_id(s):
    return "x".join(map(str, s))


def per_channel(t):
    return t.double().view(1, -1, 1, 1)


def relu64(r):
    return torch.where(r <= 0, torch.zeros_like(r), r)               # a NaN is neither: kept


def conv1(x, w):
    return F.conv2d(x, w[:, :, None, None])


def conv3(x, w, stride):
    return F.conv2d(x, w, None, stride=stride, padding=1)


def _finite(t):
    return torch.where(torch.isfinite(t), t, torch.zeros_like(t))


def _exact_in_f32(t, what):
    assert bool(((t.float().double() == t) | torch.isnan(t)).all()), f"{what} is not exact in f32"


class Conv1Case:
    """Operands of one mvn_conv1x1 launch on the CPU: x (M, Cin, H, W), w (Cout, Cin), scale, shift (Cout,) f32
    tensors of bf16-exact values; mode NONE, IDENTITY (skip (M, Cout, H, W)) or POINTWISE (skip (M, Cs, Hs, Ws),
    skip_w (Cout, Cs), skip_scale, skip_shift, skip_stride)."""

    def __init__(self, x, w, scale, shift, mode=NONE, skip=None, skip_w=None, skip_scale=None, skip_shift=None,
                 skip_stride=1):
        assert w.shape[1] == x.shape[1] and scale.shape == shift.shape == (w.shape[0],)
        self.x, self.w, self.scale, self.shift, self.mode = x, w, scale, shift, mode
        self.skip, self.skip_w, self.skip_scale, self.skip_shift, self.skip_stride = skip, skip_w, skip_scale, skip_shift, skip_stride
        if mode == POINTWISE:
            s = skip_stride
            assert (skip.shape[2] - 1) // s + 1 == x.shape[2] and (skip.shape[3] - 1) // s + 1 == x.shape[3]

    @property
    def cin(self):
        return self.x.shape[1]

    def skip_sampled(self, t=None):
        s = self.skip_stride
        return (self.skip if t is None else t)[:, :, ::s, ::s]

    def products(self):
        """Products per output and further f32 roundings of the epilogue, per skip mode (include/mvn_hip.h):
        NONE       Cin products, the fma;
        IDENTITY   Cin products, the fma, the add of the skip;
        POINTWISE  Cin + Cs products, the two fmas, the add of the two."""
        if self.mode == NONE:
            return self.cin, 1
        if self.mode == IDENTITY:
            return self.cin, 2
        return self.cin + self.skip.shape[1], 3

    def run(self, device, x_dev=None, skip_dev=None):
        from mvn_rocm import resnet
        assert bool((self.w.bfloat16().float() == self.w).all())
        xd = cl2d(self.x, device) if x_dev is None else x_dev
        args = (xd, resnet.pack_conv1x1_weight(self.w.double()).to(device), self.scale.to(device), self.shift.to(device))
        if self.mode == NONE:
            return resnet.conv1x1(*args)
        sd = cl2d(self.skip, device) if skip_dev is None else skip_dev
        if self.mode == IDENTITY:
            return resnet.conv1x1(*args, skip=sd)
        sp = (resnet.pack_conv1x1_weight(self.skip_w.double()).to(device), self.skip_scale.to(device),
              self.skip_shift.to(device))
        return resnet.conv1x1(*args, skip=sd, skip_params=sp, skip_stride=self.skip_stride)

    def abs_terms(self):
        """S of the bound, float64, non-finite values left out: the sum of the absolute terms of r."""
        S = conv1(_finite(self.x).double().abs(), self.w.double().abs()) * per_channel(self.scale).abs() + per_channel(self.shift).abs()
        if self.mode == IDENTITY:
            S = S + _finite(self.skip).double().abs()
        if self.mode == POINTWISE:
            S = S + (conv1(self.skip_sampled(_finite(self.skip)).double().abs(), self.skip_w.double().abs())
                     * per_channel(self.skip_scale).abs() + per_channel(self.skip_shift).abs())
        return S

    def pre_relu(self, f32=True):
        """r of the contract in float64, the convolutions in f32 on the CPU (``f32``) or in float64."""
        c = (lambda a, b: conv1(a, b).double()) if f32 else (lambda a, b: conv1(a.double(), b.double()))
        r = c(self.x, self.w) * per_channel(self.scale) + per_channel(self.shift)
        if self.mode == IDENTITY:
            r = r + self.skip.double()
        if self.mode == POINTWISE:
            r = r + (c(self.skip_sampled().contiguous(), self.skip_w) * per_channel(self.skip_scale)
                     + per_channel(self.skip_shift))
        return r

    def reference(self):
        """(f32 reference (M, Cout, H, W), float64 r) for operands on which no order of accumulation rounds:
        the sums of |x w| stay below 2^24 and every intermediate of the epilogue is exact in f32 (asserted)."""
        assert float(conv1(_finite(self.x).abs(), self.w.abs()).max()) < 2.0 ** 24
        pre = conv1(self.x, self.w).double() * per_channel(self.scale) + per_channel(self.shift)
        _exact_in_f32(pre, "fma(acc, scale, shift)")
        if self.mode == POINTWISE:
            xs = self.skip_sampled().contiguous()
            assert float(conv1(_finite(xs).abs(), self.skip_w.abs()).max()) < 2.0 ** 24
            _exact_in_f32(conv1(xs, self.skip_w).double() * per_channel(self.skip_scale) + per_channel(self.skip_shift),
                          "fma(acc_s, scale_s, shift_s)")
        r = self.pre_relu()
        assert not bool((torch.signbit(r) & (r == 0)).any()), "the pre-relu reference holds a -0"
        y = relu64(r)
        _exact_in_f32(y, "the reference")
        return y.float(), r


class Conv3Case:
    """Operands of one mvn_conv3x3 launch on the CPU: x (M, C, H, W), w (C, C, 3, 3), scale, shift (C,), stride."""

    def __init__(self, x, w, scale, shift, stride):
        assert tuple(w.shape) == (x.shape[1], x.shape[1], 3, 3) and stride in (1, 2)
        self.x, self.w, self.scale, self.shift, self.stride = x, w, scale, shift, stride

    def products(self):
        """9 C products, the fma."""
        return 9 * self.x.shape[1], 1

    def run(self, device, x_dev=None):
        from mvn_rocm import resnet
        assert bool((self.w.bfloat16().float() == self.w).all())
        xd = cl2d(self.x, device) if x_dev is None else x_dev
        return resnet.conv3x3(xd, resnet.pack_conv3x3_weight(self.w.double()).to(device), self.scale.to(device),
                              self.shift.to(device), stride=self.stride)

    def abs_terms(self):
        return (conv3(_finite(self.x).double().abs(), self.w.double().abs(), self.stride) * per_channel(self.scale).abs()
                + per_channel(self.shift).abs())

    def pre_relu(self, f32=True):
        acc = conv3(self.x, self.w, self.stride).double() if f32 else conv3(self.x.double(), self.w.double(), self.stride)
        return acc * per_channel(self.scale) + per_channel(self.shift)

    def reference(self):
        assert float(conv3(_finite(self.x).abs(), self.w.abs(), self.stride).max()) < 2.0 ** 24
        r = self.pre_relu()
        assert not bool((torch.signbit(r) & (r == 0)).any()), "the pre-relu reference holds a -0"
        y = relu64(r)
        _exact_in_f32(y, "the reference")
        return y.float(), r


def _ints(g, *shape):
    return torch.randint(-4, 5, shape, generator=g).float()


def integer_conv1(shape, mode, seed, pointwise=None):
    """Integers in [-4, 4], scale +-2^k, shift in quarters: every sum is exact in f32 in any order.
    ``pointwise`` = (Cs, stride, Hs, Ws) with POINTWISE."""
    M, cin, H, W, cout = shape
    g = torch.Generator().manual_seed(seed)
    x, w = _ints(g, M, cin, H, W), _ints(g, cout, cin)
    sc, sh = exact_scale_shift(seed + 1, cout)
    if mode == NONE:
        return Conv1Case(x, w, sc, sh)
    if mode == IDENTITY:
        return Conv1Case(x, w, sc, sh, IDENTITY, _ints(g, M, cout, H, W))
    cs, s, Hs, Ws = pointwise
    return Conv1Case(x, w, sc, sh, POINTWISE, _ints(g, M, cs, Hs, Ws), _ints(g, cout, cs), *exact_scale_shift(seed + 2, cout), s)


def integer_conv3(shape, seed):
    M, C, H, W, stride = shape
    g = torch.Generator().manual_seed(seed)
    return Conv3Case(_ints(g, M, C, H, W), _ints(g, C, C, 3, 3), *exact_scale_shift(seed + 1, C), stride)


def _seed(shape):
    return sum((7 * i + 3) * v for i, v in enumerate(shape))


@functools.lru_cache(maxsize=None)
def parity_conv1(shape, mode, pointwise=None):
    """The integer case of a shape and its reference, computed once and shared (read-only)."""
    case = integer_conv1(shape, mode, _seed(shape) + mode, pointwise)
    return (case,) + case.reference()


@functools.lru_cache(maxsize=None)
def parity_conv3(shape):
    case = integer_conv3(shape, _seed(shape))
    return (case,) + case.reference()


def _rand_scale_shift(g, n):
    scale = (0.75 + 0.5 * torch.rand(n, generator=g)) * torch.where(torch.arange(n) % 5 == 2, -1.0, 1.0)
    return scale, 0.2 * torch.randn(n, generator=g)


def random_conv1(shape, mode, seed, pointwise=None):
    """randn inputs, weights of std 3 sqrt(2 / (Cin + Cout)), scale in [0.75, 1.25] of both signs; bf16-exact."""
    M, cin, H, W, cout = shape
    g = torch.Generator().manual_seed(seed)
    x = bf16r(torch.randn(M, cin, H, W, generator=g))
    w = bf16r(torch.randn(cout, cin, generator=g) * (2.0 / (cin + cout)) ** 0.5 * 3)
    sc, sh = _rand_scale_shift(g, cout)
    if mode == NONE:
        return Conv1Case(x, w, sc, sh)
    if mode == IDENTITY:
        return Conv1Case(x, w, sc, sh, IDENTITY, bf16r(torch.randn(M, cout, H, W, generator=g)))
    cs, s, Hs, Ws = pointwise
    skip = bf16r(torch.randn(M, cs, Hs, Ws, generator=g))
    ws = bf16r(torch.randn(cout, cs, generator=g) * (2.0 / (cs + cout)) ** 0.5 * 3)
    return Conv1Case(x, w, sc, sh, POINTWISE, skip, ws, *_rand_scale_shift(g, cout), s)


def random_conv3(shape, seed):
    M, C, H, W, stride = shape
    g = torch.Generator().manual_seed(seed)
    x = bf16r(torch.randn(M, C, H, W, generator=g))
    w = bf16r(torch.randn(C, C, 3, 3, generator=g) * (2.0 / (18 * C)) ** 0.5 * 3)
    return Conv3Case(x, w, *_rand_scale_shift(g, C), stride)


def check_bound(case, got, what):
    """|got - ref| <= 2^-8 |ref| + gamma S per element: half a bf16 ulp of the one rounding plus the worst-case
    f32 bound of the sums, gamma = (products per output + further f32 roundings of the epilogue) 2^-24
    (``case.products``), S the sum of the absolute terms, ref the float64 restatement.  The same convolution in
    f32 on the CPU must sit within 0.05 of gamma S, so the bar is a bound for these inputs and no
    measurement.  Returns the worst fraction of the bar."""
    n, extra = case.products()
    gamma, S = (n + extra) * 2.0 ** -24, case.abs_terms()
    r = case.pre_relu(f32=False)
    ref = relu64(r)
    cpu_frac = float(((case.pre_relu(f32=True) - r).abs() / (gamma * S)).max())
    frac = float(((got.double() - ref).abs() / (2.0 ** -8 * ref.abs() + gamma * S)).max())
    print(f"{what}: worst |got - ref| / bar = {frac:.4f}; the f32 CPU convolution at {cpu_frac:.4f} of gamma S")
    assert cpu_frac <= 0.05, "the f32 CPU convolution is not far inside gamma S: the bar is no bound for these inputs"
    assert frac <= 1.0
    return frac


# ----------------------------------------------------------------------------- index weights, unpackers
def index_weight1(cout, cin):
    """A bf16-exact (Cout, Cin) weight that encodes its own index: the exponent holds ci % 8 (the slot within a
    lane's 8 K-values) and co // 128, the significand and the sign hold co % 128 mixed with ci // 8 (the lane
    group and the K-step).  Two slots that a wrong read could confuse differ in value."""
    co, ci = torch.arange(cout).view(-1, 1), torch.arange(cin).view(1, -1)
    mant = ((co % 64) * 37 + (ci // 8) * 53) % 128
    sign = torch.where(co % 128 >= 64, -1.0, 1.0)
    w = (sign * (1.0 + mant.double() / 128) * torch.exp2((ci % 8 + 8 * (co // 128) - 64).double())).float()
    assert bool((w.bfloat16().float() == w).all())
    return w.contiguous()


def index_weight3(C):
    """As ``index_weight1`` for (C, C, 3, 3): the exponent also holds the tap."""
    tap = torch.arange(9).view(1, 1, 3, 3)
    w = index_weight1(C, C).double().view(C, C, 1, 1) * torch.exp2((16 * tap - 32).double())
    w = w.float().contiguous()
    assert bool((w.bfloat16().float() == w).all()) and bool(torch.isfinite(w).all()) and bool((w != 0).all())
    return w


def unpack_conv1x1(packed, cout, cin):
    """The (cout, cin) weight from the documented layout (include/mvn_hip.h):
    [kp][m][lane][j] = w[16 m + (lane & 15)][32 kp + 8 (lane >> 4) + j]."""
    assert tuple(packed.shape) == (cin // 32, cout // 16, 64, 8) and packed.dtype == torch.bfloat16
    a = unpack_mfma_a(packed)                                    # (KP, cout rows, 32 K-slots)
    return a.permute(1, 0, 2).reshape(cout, cin)


def unpack_conv3x3(packed, C):
    """The (C, C, 3, 3) weight from the documented layout:
    [tap = ky*3 + kx][kp][m][lane][j] = w[16 m + (lane & 15)][32 kp + 8 (lane >> 4) + j][ky][kx]."""
    assert tuple(packed.shape) == (9, C // 32, C // 16, 64, 8) and packed.dtype == torch.bfloat16
    a = unpack_mfma_a(packed)                                    # (9, KP, C rows = co, 32 K-slots = ci % 32)
    return a.permute(2, 1, 3, 0).reshape(C, C, 3, 3)


def element1(packed, kp, m, lane, j):
    """The documented element formula of mvn_conv1x1 read literally: ((co, ci), value)."""
    return (16 * m + (lane & 15), 32 * kp + 8 * (lane >> 4) + j), float(packed[kp, m, lane, j])


def element3(packed, tap, kp, m, lane, j):
    """That of mvn_conv3x3: ((co, ci, ky, kx), value)."""
    return (16 * m + (lane & 15), 32 * kp + 8 * (lane >> 4) + j, tap // 3, tap % 3), float(packed[tap, kp, m, lane, j])


# ----------------------------------------------------------------------------- stand-in modules
class Bottleneck(nn.Module):
    """The reference's Bottleneck by attribute names and forward order (1x1, 3x3 carrying the stride, 1x1 to
    four times the width; BatchNorms; the residual through ``downsample`` where there is one), from torch.nn."""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * self.expansion, kernel_size=1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        return self.relu(out + (x if self.downsample is None else self.downsample(x)))


def make_block(inplanes, planes, stride=1, seed=0):
    """A randomised eval-mode stand-in block, with a downsample where the reference's ``_make_layer`` puts one."""
    down = None
    if stride != 1 or inplanes != planes * Bottleneck.expansion:
        down = nn.Sequential(nn.Conv2d(inplanes, planes * Bottleneck.expansion, kernel_size=1, stride=stride, bias=False),
                             nn.BatchNorm2d(planes * Bottleneck.expansion))
    return randomise2d(Bottleneck(inplanes, planes, stride, down), seed)


def make_layer(inplanes, planes, blocks, stride):
    layers = [make_block(inplanes, planes, stride)]
    layers += [make_block(planes * Bottleneck.expansion, planes) for _ in range(1, blocks)]
    return nn.Sequential(*layers)


TRUNK_M, TRUNK_IMAGE = 3, (40, 56)                  # maps of 10 x 14, 5 x 7, 3 x 4 and 2 x 2
TRUNK_COUT = 256


class StandInTrunkBackbone(nn.Module):
    """The reference's PoseResNet by attribute names and forward order: its stem (7x7 stride-2 convolution,
    BatchNorm, ReLU, 3x3 stride-2 max pool), four stages of Bottleneck at strides 1, 2, 2, 2 (the first of
    two blocks, so both kinds of residual occur; 64-channel middles, ending at 256 channels), three deconv
    triples, final_layer and a confidence head."""

    def __init__(self, joints=17):
        super().__init__()
        from deconv_project_kit import ConfidenceHead
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = make_layer(64, 64, 2, 1)       # 64 -> 256 (downsample, stride 1), 256 -> 256 (identity)
        self.layer2 = make_layer(256, 64, 1, 2)      # 256 -> 256 at stride 2: a downsample that keeps the width
        self.layer3 = make_layer(256, 64, 2, 2)
        self.layer4 = make_layer(256, 64, 1, 2)
        self.vol_confidences = ConfidenceHead(TRUNK_COUT, 32)
        self.alg_confidences = ConfidenceHead(TRUNK_COUT, joints)
        layers, cin = [], TRUNK_COUT
        for _ in range(3):
            layers += [nn.ConvTranspose2d(cin, 256, 4, stride=2, padding=1, output_padding=0, bias=False),
                       nn.BatchNorm2d(256), nn.ReLU(inplace=True)]
            cin = 256
        self.deconv_layers = nn.Sequential(*layers)
        self.final_layer = nn.Conv2d(256, joints, 1)

    def stem(self, x):
        return self.maxpool(self.relu(self.bn1(self.conv1(x))))

    def blocks(self):
        return [b for name in ("layer1", "layer2", "layer3", "layer4") for b in getattr(self, name)]

    def trunk(self, x):
        return self.layer4(self.layer3(self.layer2(self.layer1(self.stem(x)))))


@functools.lru_cache(maxsize=None)
def stand_in_backbone():
    """The randomised stand-in on the CPU, built once (read-only: copy before moving it)."""
    net = randomise2d(StandInTrunkBackbone(), seed=52, bias=0.02)
    g = torch.Generator().manual_seed(53)
    with torch.no_grad():
        for head in (net.vol_confidences, net.alg_confidences):
            lin = head.head[0]
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=g) * 0.1)
            lin.bias.copy_(torch.randn(lin.bias.shape, generator=g) * 0.1)
    return net.eval()


@functools.lru_cache(maxsize=None)
def trunk_images():
    return torch.randn(TRUNK_M, 3, *TRUNK_IMAGE, generator=torch.Generator().manual_seed(54))


def block_reference(block, x):
    """The stand-in block on the CPU as the three launches compute it, in float64 with every convolution's
    operands rounded to bf16 and the activations rounded to bf16 between the convolutions: x (M, Cin, H, W)
    bf16-exact f32.  Returns (the float64 pre-rounding output, the bound per element): for each convolution
    one bf16 ulp of its output (2^-7 |value|: the half-ulp rounding of the kernel and of this restatement may
    fall on either side) plus gamma S, carried through the convolutions behind it by their absolute weights."""
    def fold(conv, bn):
        s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
        return bf16r(conv.weight.detach()).double(), s.float().double(), ((0 - bn.running_mean.double()) * s + bn.bias.double()).float().double()

    def conv(h, w, s, t, stride, pad, err):
        """(r, the bound on r): h exact input (float64), err the bound on the kernel's deviation from h."""
        n = w[0].numel()
        acc = F.conv2d(h, w, None, stride=stride, padding=pad)
        S = F.conv2d(h.abs(), w.abs(), None, stride=stride, padding=pad) * s.abs().view(1, -1, 1, 1) + t.abs().view(1, -1, 1, 1)
        carried = F.conv2d(err, w.abs(), None, stride=stride, padding=pad) * s.abs().view(1, -1, 1, 1)
        return acc * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1), S, carried, n

    with torch.no_grad():
        u = 2.0 ** -24
        x64 = x.double()
        zero = torch.zeros_like(x64)
        w1, s1, t1 = fold(block.conv1, block.bn1)
        r, S, c, n = conv(x64, w1, s1, t1, 1, 0, zero)
        e1 = c + (n + 1) * u * S
        h1 = bf16r(relu64(r)).double()
        e1 = e1 + 2.0 ** -7 * h1.abs() + 2.0 ** -7 * e1      # the kernel rounds a value within e1 of r
        w2, s2, t2 = fold(block.conv2, block.bn2)
        r, S, c, n = conv(h1, w2, s2, t2, block.stride, 1, e1)
        e2 = c + (n + 1) * u * (S + c)
        h2 = bf16r(relu64(r)).double()
        e2 = e2 + 2.0 ** -7 * h2.abs() + 2.0 ** -7 * e2
        w3, s3, t3 = fold(block.conv3, block.bn3)
        r, S, c, n = conv(h2, w3, s3, t3, 1, 0, e2)
        if block.downsample is None:
            r, S, extra = r + x64, S + x64.abs(), 2
        else:
            wd, sd, td = fold(block.downsample[0], block.downsample[1])
            rd, Sd, _, nd = conv(x64, wd, sd, td, block.stride, 0, zero)
            r, S, n, extra = r + rd, S + Sd, n + nd, 3
        e3 = c + (n + extra) * u * (S + c)
        y = relu64(r)
        return y, e3 + 2.0 ** -7 * y.abs() + 2.0 ** -7 * e3


class StandInTrunkModel(nn.Module):
    """The attributes of VolumetricTriangulationNet that VolumetricModelEval reads, around the stand-in backbone."""

    def __init__(self, joints, multiplier):
        super().__init__()
        from v2v_kit import V2VModel
        self.backbone = StandInTrunkBackbone(joints)
        self.process_features = nn.Sequential(nn.Conv2d(256, 32, 1))
        self.volume_net = V2VModel(32, joints)
        self.volume_aggregation_method = "softmax"
        self.volume_multiplier = multiplier
        self.volume_softmax = True


@functools.lru_cache(maxsize=None)
def stand_in_trunk_model(joints=5, multiplier=10.0):
    """The randomised stand-in model on the CPU, built once (read-only: copy before moving it); its backbone
    has the weights of ``stand_in_backbone`` except for the ``joints``-wide layers."""
    from v2v_kit import randomise
    net = StandInTrunkModel(joints, multiplier)
    randomise2d(net.backbone, seed=52, bias=0.02)
    randomise2d(net.process_features, seed=55, bias=0.1)
    randomise(net.volume_net, seed=2026)
    g = torch.Generator().manual_seed(53)
    with torch.no_grad():
        for head in (net.backbone.vol_confidences, net.backbone.alg_confidences):
            lin = head.head[0]
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=g) * 0.1)
            lin.bias.copy_(torch.randn(lin.bias.shape, generator=g) * 0.1)
    return net.eval()
