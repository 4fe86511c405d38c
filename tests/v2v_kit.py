"""What the V2V tests share (tests/test_gpu_v2v_{res3d,interior,deep}.py, their *_api.py files,
test_feature_conv_api.py, test_gpu_volumetric_eval.py): the stand-in V2V model, the bit and layout
helpers, and the method of the conv and upsample tests once, on a literal record per channel width.

The method: operands for which the kernel's f32 arithmetic is exact in any summation order
(integers in [-4, 4], scales +-2^k, shifts in quarters; impulse lattices with one product per
output), compared bit for bit with the arithmetic contract of include/mvn_hip.h restated in float64
(+0 where r <= 0, NaN kept, cast to f32, then ``.bfloat16()``; the reference holds no -0), plus
random data against that restatement with the contract's own bound.

Nothing here is read from the code under test: the records below are written out, the unpackers
follow the documented layouts.  Not a test module and not a conftest.  Reads nothing outside the
repository.
"""
import copy
import dataclasses
import functools

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

NONE, IDENTITY, POINTWISE = 0, 1, 2
MODE_NAME = {NONE: "none", IDENTITY: "identity", POINTWISE: "pointwise"}


# ----------------------------------------------------------------------------- stand-ins
class Basic3DBlock(nn.Module):
    """The reference's Basic3DBlock (v2v.py:7-17), from torch.nn."""

    def __init__(self, cin, cout, k):
        super().__init__()
        self.block = nn.Sequential(nn.Conv3d(cin, cout, k, 1, (k - 1) // 2), nn.BatchNorm3d(cout), nn.ReLU(True))

    def forward(self, x):
        return self.block(x)


class Res3DBlock(nn.Module):
    """The reference's Res3DBlock (v2v.py:20-42), from torch.nn, with its attribute names."""

    def __init__(self, cin, cout, bias=True):
        super().__init__()
        self.res_branch = nn.Sequential(nn.Conv3d(cin, cout, 3, 1, 1, bias=bias), nn.BatchNorm3d(cout), nn.ReLU(True),
                                        nn.Conv3d(cout, cout, 3, 1, 1, bias=bias), nn.BatchNorm3d(cout))
        self.skip_con = nn.Sequential() if cin == cout else nn.Sequential(nn.Conv3d(cin, cout, 1, 1, 0, bias=bias),
                                                                          nn.BatchNorm3d(cout))

    def forward(self, x):
        return F.relu(self.res_branch(x) + self.skip_con(x), True)


class Pool3DBlock(nn.Module):
    def __init__(self, k):
        super().__init__()
        self.k = k

    def forward(self, x):
        return F.max_pool3d(x, kernel_size=self.k, stride=self.k)


class Upsample3DBlock(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.block = nn.Sequential(nn.ConvTranspose3d(cin, cout, 2, 2), nn.BatchNorm3d(cout), nn.ReLU(True))

    def forward(self, x):
        return self.block(x)


class EncoderDecorder(nn.Module):
    """The reference's EncoderDecorder (v2v.py:69-138): attribute names and forward."""

    def __init__(self):
        super().__init__()
        self.encoder_pool1, self.encoder_res1 = Pool3DBlock(2), Res3DBlock(32, 64)
        self.encoder_pool2, self.encoder_res2 = Pool3DBlock(2), Res3DBlock(64, 128)
        self.encoder_pool3, self.encoder_res3 = Pool3DBlock(2), Res3DBlock(128, 128)
        self.encoder_pool4, self.encoder_res4 = Pool3DBlock(2), Res3DBlock(128, 128)
        self.encoder_pool5, self.encoder_res5 = Pool3DBlock(2), Res3DBlock(128, 128)
        self.mid_res = Res3DBlock(128, 128)
        self.decoder_res5, self.decoder_upsample5 = Res3DBlock(128, 128), Upsample3DBlock(128, 128)
        self.decoder_res4, self.decoder_upsample4 = Res3DBlock(128, 128), Upsample3DBlock(128, 128)
        self.decoder_res3, self.decoder_upsample3 = Res3DBlock(128, 128), Upsample3DBlock(128, 128)
        self.decoder_res2, self.decoder_upsample2 = Res3DBlock(128, 128), Upsample3DBlock(128, 64)
        self.decoder_res1, self.decoder_upsample1 = Res3DBlock(64, 64), Upsample3DBlock(64, 32)
        self.skip_res1, self.skip_res2 = Res3DBlock(32, 32), Res3DBlock(64, 64)
        self.skip_res3, self.skip_res4, self.skip_res5 = Res3DBlock(128, 128), Res3DBlock(128, 128), Res3DBlock(128, 128)

    def forward(self, x):
        s1 = self.skip_res1(x)
        x = self.encoder_res1(self.encoder_pool1(x))
        s2 = self.skip_res2(x)
        x = self.encoder_res2(self.encoder_pool2(x))
        s3 = self.skip_res3(x)
        x = self.encoder_res3(self.encoder_pool3(x))
        s4 = self.skip_res4(x)
        x = self.encoder_res4(self.encoder_pool4(x))
        s5 = self.skip_res5(x)
        x = self.encoder_res5(self.encoder_pool5(x))
        x = self.mid_res(x)
        x = self.decoder_upsample5(self.decoder_res5(x)) + s5
        x = self.decoder_upsample4(self.decoder_res4(x)) + s4
        x = self.decoder_upsample3(self.decoder_res3(x)) + s3
        x = self.decoder_upsample2(self.decoder_res2(x)) + s2
        return self.decoder_upsample1(self.decoder_res1(x)) + s1


class V2VModel(nn.Module):
    """The reference's V2VModel (v2v.py:141-169): attribute names and forward."""

    def __init__(self, cin, J):
        super().__init__()
        self.front_layers = nn.Sequential(Basic3DBlock(cin, 16, 7), Res3DBlock(16, 32), Res3DBlock(32, 32),
                                          Res3DBlock(32, 32))
        self.encoder_decoder = EncoderDecorder()
        self.back_layers = nn.Sequential(Res3DBlock(32, 32), Basic3DBlock(32, 32, 1), Basic3DBlock(32, 32, 1))
        self.output_layer = nn.Conv3d(32, J, 1)

    def forward(self, x):
        return self.output_layer(self.back_layers(self.encoder_decoder(self.front_layers(x))))


def randomise(module, seed, bias=0.1):
    """Xavier-normal conv weights (v2v.py:171-180), small biases, BatchNorm statistics of a
    trained layer's order of magnitude; eval mode."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, (nn.Conv3d, nn.ConvTranspose3d)):
                rf = m.weight[0, 0].numel()
                fan = (m.weight.shape[0] + m.weight.shape[1]) * rf
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan) ** 0.5)
                if m.bias is not None:
                    m.bias.copy_(torch.randn(m.bias.shape, generator=g) * bias)
            elif isinstance(m, nn.BatchNorm3d):
                n = m.num_features
                m.weight.copy_(0.75 + 0.5 * torch.rand(n, generator=g))
                m.bias.copy_(0.2 * torch.randn(n, generator=g))
                m.running_mean.copy_(0.2 * torch.randn(n, generator=g))
                m.running_var.copy_(0.75 + 0.5 * torch.rand(n, generator=g))
    return module.eval()


J = 17


@functools.lru_cache(maxsize=None)
def stand_in_model():
    return randomise(V2VModel(32, J), seed=2024, bias=0.02)


def bf16_operand_model(m):
    """The stand-in on the CPU with every conv operand rounded to bf16: weights rounded once, the
    input of every Conv3d / ConvTranspose3d rounded by a forward pre-hook; everything else f32."""
    mb = copy.deepcopy(m)
    with torch.no_grad():
        for mod in mb.modules():
            if isinstance(mod, (nn.Conv3d, nn.ConvTranspose3d)):
                mod.weight.copy_(bf16r(mod.weight))
                mod.register_forward_pre_hook(lambda _m, args: (bf16r(args[0]),))
    return mb


E2E_SIDE = 2500.0
E2E_MULT = 10.0


def e2e_case(device):
    """Blob-like input (synth.blob_volumes in the first 17 of 32 channels, unit noise elsewhere)
    and a multiplier that makes the stand-in's logits peaked."""
    from mvn_rocm import synth, volumetric
    V = 32
    coords = volumetric.build_coord_volumes(np.array([[10.0, -20.0, 900.0]]), E2E_SIDE, V, theta=[0.3], device=device)
    blobs = synth.blob_volumes(coords, J, seed=4).cpu()
    x = torch.cat([blobs, 0.1 * torch.randn(1, 32 - J, V, V, V, generator=torch.Generator().manual_seed(2))], dim=1)
    return bf16r(x), coords


# ----------------------------------------------------------------------------- bits and layouts
def bits(t):
    """The bit pattern of a bf16 / f32 tensor as a numpy unsigned array (on the host)."""
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy().view(np.uint32)
    assert t.dtype == torch.bfloat16
    return t.view(torch.int16).numpy().view(np.uint16)


def assert_same_bits(got, want):
    a, b = bits(got), bits(want)
    assert a.shape == b.shape, (a.shape, b.shape)
    bad = a != b
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} elements differ in their bits"


def cl(x, device):
    """(B, C, V, V, V) f32 holding bf16-exact values -> the kernel's (B, V, V, V, C) bf16 volume."""
    xb = x.bfloat16()
    assert bool(((xb.float() == x) | torch.isnan(x)).all()), "the test's volume is not exact in bf16"
    return xb.permute(0, 2, 3, 4, 1).contiguous().to(device)


def ncdhw(y_cl):
    """The kernel's (B, V, V, V, C) result as (B, C, V, V, V) on the CPU."""
    return y_cl.cpu().permute(0, 4, 1, 2, 3).contiguous()


def bf16r(t):
    return t.float().bfloat16().float()


def bf16_full(shape, g):
    """Normal bf16 values with full 8-bit significands (random normal, rounded to bf16)."""
    v = torch.randn(shape, generator=g).bfloat16().float()
    return torch.where(v.abs() > 2.0 ** -100, v, torch.ones_like(v))


def per_channel(t):
    return t.double().view(1, -1, 1, 1, 1)


def lattice_reference(x, w, scale, pad):
    """At most one product per output (asserted), so the float64 conv IS that product: times
    scale in float64, rounded once to f32 (the kernel's fma with a zero shift)."""
    k = 2 * pad + 1
    hits = F.conv3d((x != 0).double(), torch.ones(1, x.shape[1], k, k, k, dtype=torch.float64), padding=pad)
    assert float(hits.max()) == 1.0
    return (F.conv3d(x.double(), w.double(), None, padding=pad) * per_channel(scale)).float()


def lattice_input(cin, off, g, B=2, V=16):
    """Impulses at the voxels off, off + 3, ... of every axis, one channel each, every channel used."""
    x = torch.zeros((B, cin, V, V, V))
    n = torch.arange(off, V, 3).numel()
    ch = (torch.arange(B * n ** 3).view(B, n, n, n) * 5 + 11 * torch.arange(B).view(B, 1, 1, 1)) % cin
    sub = torch.zeros(B, cin, n, n, n).scatter_(1, ch.unsqueeze(1), bf16_full((B, 1, n, n, n), g))
    x[:, :, off::3, off::3, off::3] = sub
    assert int((x != 0).sum()) == B * n ** 3 and len(set(ch.flatten().tolist())) == cin      # every channel used
    return x


# 3^3 boxes pairwise disjoint at V = 32: both corners, either side of the x seam 11 | 12, of the y
# seam 7 | 8 and of the z seam 15 | 16 (tiles are 4 x 8 x 16)
NAN_VOXELS = ((0, 0, 0), (31, 31, 31), (11, 20, 5), (12, 20, 27), (24, 7, 8), (24, 8, 24), (20, 27, 15), (4, 27, 16))
INF_VOXELS = ((12, 12, 12, 5, float("inf")), (22, 20, 7, 13, float("-inf")))      # x, y, z, channel, value
N_BOX = 2 * 2 ** 3 + 6 * 3 ** 3


def box_mask(V, voxels, pad):
    m = np.zeros((V, V, V), bool)
    for x, y, z in voxels:
        m[max(x - pad, 0):x + pad + 1, max(y - pad, 0):y + pad + 1, max(z - pad, 0):z + pad + 1] = True
    return m


SENTINEL = 0x7FA5            # a NaN with its own payload: relu of finite data never gives it
BAND = 64 * 1024 // 2        # 64 KiB of bf16 on either side


def banded(t, fill_nan=True):
    """(the larger buffer, the view of ``t``'s shape inside it): NaN bands around an input,
    sentinel bands (and sentinel contents) around an output when ``t`` is a shape."""
    if isinstance(t, torch.Tensor):
        big = torch.full((BAND + t.numel() + BAND,), float("nan"), dtype=torch.bfloat16, device=t.device)
        view = big[BAND:BAND + t.numel()].view(t.shape)
        view.copy_(t)
        return big, view
    shape, device = t
    n = int(np.prod(shape))
    big = torch.full((BAND + n + BAND,), SENTINEL, dtype=torch.int16, device=device)
    return big, big[BAND:BAND + n].view(torch.bfloat16).view(shape)


def bands_intact(big, n, inside_written):
    ok = bool((big[:BAND] == SENTINEL).all()) and bool((big[BAND + n:] == SENTINEL).all())
    return ok and (not inside_written or not bool((big[BAND:BAND + n] == SENTINEL).any()))


# ----------------------------------------------------------------------------- the conv, per width
def exact_scale_shift(seed, n):
    """Per-channel scale = +-2^k (k in -2..1, both signs present) and shift = a multiple of 1/4
    (never -0)."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(-2, 2, (n,), generator=g).float()
    sign = torch.where(torch.arange(n) % 3 == 1, -1.0, 1.0)
    scale = sign * torch.exp2(k)
    shift = torch.randint(-8, 9, (n,), generator=g).float() / 4 + 0.0
    assert not bool((torch.signbit(shift) & (shift == 0)).any())
    assert bool((scale < 0).any()) and bool((scale > 0).any())
    return scale, shift


@dataclasses.dataclass(frozen=True)
class Level:
    """One channel width of the 3x3x3 conv + folded BN + skip + ReLU, written out (not read from
    mvn_rocm.v2v): the mvn_rocm.v2v names are looked up when a case runs."""
    co: int                  # output channels
    cins: tuple              # input widths the kernel takes
    skip_cin: int            # the pointwise skip's input width (the identity skip's is co)
    conv: str                # v2v function of one launch
    packer: str              # v2v packer of the (co, cin, 3, 3, 3) weight
    skip_packer: str         # v2v packer of the (co, skip_cin) pointwise-skip weight
    extent: object           # V -> whether the kernel takes (B, V, V, V, C) volumes

    def skip_c(self, mode):
        return {NONE: 0, IDENTITY: self.co, POINTWISE: self.skip_cin}[mode]

    def pack(self, w, device):
        from mvn_rocm import v2v
        assert bool((w.bfloat16().float() == w).all())
        return getattr(v2v, self.packer)(w.double()).to(device)

    def pack_skip(self, ws, device):
        from mvn_rocm import v2v
        return getattr(v2v, self.skip_packer)(ws.double()).to(device)

    def case(self, *args, **kwargs):
        return ConvCase(self, *args, **kwargs)

    def exact_scale_shift(self, seed, n=None):
        return exact_scale_shift(seed, self.co if n is None else n)

    def integer_case(self, B, V, cin, mode, seed):
        g = torch.Generator().manual_seed(seed)
        x = torch.randint(-4, 5, (B, cin, V, V, V), generator=g).float()
        w = torch.randint(-4, 5, (self.co, cin, 3, 3, 3), generator=g).float()
        case = ConvCase(self, x, w, *exact_scale_shift(seed + 1, self.co), mode)
        if mode != NONE:
            case.skip = torch.randint(-4, 5, (B, self.skip_c(mode), V, V, V), generator=g).float()
        if mode == POINTWISE:
            case.ws = torch.randint(-4, 5, (self.co, self.skip_cin), generator=g).float()
            case.scale_s, case.shift_s = exact_scale_shift(seed + 2, self.co)
        return case

    def parity_case(self, B, V, cin, mode):
        return _parity_case(self, B, V, cin, mode)

    def random_case(self, B, V, cin, mode, seed, x=None):
        co = self.co
        g = torch.Generator().manual_seed(seed)
        if x is None:
            x = bf16r(torch.randn(B, cin, V, V, V, generator=g))
        w = bf16r(torch.randn(co, cin, 3, 3, 3, generator=g) * (2.0 / (27 * (cin + co))) ** 0.5 * 3)
        scale = (0.75 + 0.5 * torch.rand(co, generator=g)) * torch.where(torch.arange(co) % 5 == 2, -1.0, 1.0)
        case = ConvCase(self, x, w, scale, 0.2 * torch.randn(co, generator=g), mode)
        if mode != NONE:
            case.skip = bf16r(torch.randn(B, self.skip_c(mode), V, V, V, generator=g))
        if mode == POINTWISE:
            case.ws = bf16r(torch.randn(co, self.skip_cin, generator=g) * 0.2)
            case.scale_s = 0.75 + 0.5 * torch.rand(co, generator=g)
            case.shift_s = 0.2 * torch.randn(co, generator=g)
        return case


RES3D = Level(32, (16, 32), 16, "v2v_conv3", "pack_conv3_weight", "pack_pointwise_skip_weight",
              lambda V: 16 <= V <= 256 and V % 16 == 0)
WIDE = Level(64, (32, 64), 32, "v2v_conv3_wide", "pack_conv3_wide_weight", "pack_pointwise_skip_wide_weight",
             lambda V: 16 <= V <= 128 and V % 16 == 0)
DEEP = Level(128, (64, 128), 64, "v2v_conv3_deep", "pack_conv3_deep_weight", "pack_pointwise_skip_deep_weight",
             lambda V: 1 <= V <= 64)


class ConvCase:
    """Operands of one launch of a level's conv on the CPU (f32 tensors holding bf16-exact values)."""

    def __init__(self, level, x, w, scale, shift, mode=NONE, skip=None, ws=None, scale_s=None, shift_s=None):
        self.level = level
        self.x, self.w, self.scale, self.shift, self.mode = x, w, scale, shift, mode
        self.skip, self.ws, self.scale_s, self.shift_s = skip, ws, scale_s, shift_s

    def args(self, device, x_dev=None, skip_dev=None):
        lv = self.level
        assert self.x.shape[1] in lv.cins and lv.extent(self.x.shape[2])
        a = [cl(self.x, device) if x_dev is None else x_dev, lv.pack(self.w, device), self.scale.to(device),
             self.shift.to(device)]
        if self.mode != NONE:
            a.append(cl(self.skip, device) if skip_dev is None else skip_dev)
        if self.mode == POINTWISE:
            a += [lv.pack_skip(self.ws, device), self.scale_s.to(device), self.shift_s.to(device)]
        return a

    def run(self, device, x_dev=None, skip_dev=None):
        from mvn_rocm import v2v
        return getattr(v2v, self.level.conv)(*self.args(device, x_dev, skip_dev))

    def abs_sum(self):
        """The largest sum of |x w| over an output, non-finite voxels left out."""
        finite = torch.where(torch.isfinite(self.x), self.x, torch.zeros_like(self.x))
        return float(F.conv3d(finite.abs(), self.w.abs(), None, padding=1).max())

    def pre_relu(self, exact=True):
        """r of the contract in float64; the convs in f32 on the CPU when ``exact`` (guarded: the sum
        of |x w| is below 2^24, so no order of accumulation rounds), else in float64."""
        x, w, lv = self.x, self.w, self.level
        if exact:
            assert self.abs_sum() < 2.0 ** 24
            acc = F.conv3d(x, w, None, padding=1).double()
        else:
            acc = F.conv3d(x.double(), w.double(), None, padding=1)
        r = acc * per_channel(self.scale) + per_channel(self.shift)
        if self.mode == IDENTITY:
            r = r + self.skip.double()
        elif self.mode == POINTWISE:
            w1 = self.ws.view(lv.co, lv.skip_cin, 1, 1, 1)
            acc_s = F.conv3d(self.skip, w1).double() if exact else F.conv3d(self.skip.double(), w1.double())
            r = r + (acc_s * per_channel(self.scale_s) + per_channel(self.shift_s))
        return r

    def reference(self):
        """(bf16 reference, float64 pre-relu r)."""
        r = self.pre_relu()
        assert not bool((torch.signbit(r) & (r == 0)).any()), "the pre-relu reference holds a -0"
        y = torch.where(r <= 0, torch.zeros_like(r), r)            # a NaN is neither: kept
        return y.float().bfloat16(), r


@functools.lru_cache(maxsize=None)
def _parity_case(level, B, V, cin, mode):
    case = level.integer_case(B, V, cin, mode, seed=1000 * B + V + 7 * cin + mode)
    ref, r = case.reference()
    return case, ref, r


def check_bound(case, got, what):
    """|got - ref| <= 2^-8 |ref| + gamma S per element, gamma = (27 Cin + Cin_skip + 4) 2^-24 (half a
    bf16 ulp plus the worst-case f32 summation bound of the contract), ref the
    float64 restatement, S the sum of the absolute terms; returns the worst fraction of the bar.  The
    same conv in f32 on the CPU must sit far inside gamma S (a bound, not a measurement)."""
    lv = case.level
    cin = case.x.shape[1]
    gamma = (27 * cin + lv.skip_c(case.mode) + 4) * 2.0 ** -24
    r = case.pre_relu(exact=False)
    ref = torch.where(r <= 0, torch.zeros_like(r), r)
    S = F.conv3d(case.x.double().abs(), case.w.double().abs(), None, padding=1) * per_channel(case.scale).abs() \
        + per_channel(case.shift).abs()
    if case.mode == IDENTITY:
        S = S + case.skip.double().abs()
    elif case.mode == POINTWISE:
        S = S + F.conv3d(case.skip.double().abs(), case.ws.double().abs().view(lv.co, lv.skip_cin, 1, 1, 1)) \
            * per_channel(case.scale_s).abs() + per_channel(case.shift_s).abs()
    r32 = case.pre_relu(exact=True)                     # the f32 CPU conv (the guard holds: finite data)
    cpu_frac = float(((r32 - r).abs() / (gamma * S)).max())
    bar = 2.0 ** -8 * ref.abs() + gamma * S
    frac = float(((got.double() - ref).abs() / bar).max())
    print(f"{what}: worst |got - ref| / bar = {frac:.4f}; f32 CPU conv at {cpu_frac:.4f} of gamma S")
    assert cpu_frac <= 0.05, "the f32 CPU conv is not far inside gamma S: the bar is no bound for these inputs"
    assert frac <= 1.0
    return frac


# ----------------------------------------------------------------------------- the upsample, per kernel
@dataclasses.dataclass(frozen=True)
class Up:
    """One of the two ConvTranspose3d(cin, cout, 2, 2) + BN + ReLU (+ skip) kernels, written out."""
    cin: int
    couts: tuple
    fn: str                  # v2v function of one launch
    packer: str              # v2v packer of the (cin, cout, 2, 2, 2) weight

    def case(self, *args, **kwargs):
        return UpCase(self, *args, **kwargs)

    def integer_case(self, B, V, cout, seed, negative_pre):
        """Integers in [-4, 4]: sums stay <= cin * 16.  ``negative_pre``: every scale negative and the
        shift non-positive with non-negative products, so every pre-activation is <= 0 while the skip
        is positive: a ReLU after the add would give pre + skip, the contract gives skip."""
        g = torch.Generator().manual_seed(seed)
        x = torch.randint(-4, 5, (B, self.cin, V, V, V), generator=g).float()
        w = torch.randint(-4, 5, (self.cin, cout, 2, 2, 2), generator=g).float()
        scale, shift = exact_scale_shift(seed + 1, cout)
        skip = torch.randint(-4, 5, (B, cout, 2 * V, 2 * V, 2 * V), generator=g).float()
        if negative_pre:
            x, w = x.abs(), w.abs()                                  # acc >= 0
            scale, shift = -scale.abs(), -shift.abs()                # pre <= 0
            skip = skip.abs() + 1.0                                  # skip > 0
        return UpCase(self, x, w, scale, shift, skip)


UP_WIDE = Up(64, (32,), "upsample2_add", "pack_upsample_weight")
UP_DEEP = Up(128, (64, 128), "upsample2_add_deep", "pack_upsample_deep_weight")


class UpCase:
    """Operands of one upsample launch on the CPU (f32 tensors of bf16-exact values)."""

    def __init__(self, up, x, w, scale, shift, skip=None):
        self.up = up
        self.x, self.w, self.scale, self.shift, self.skip = x, w, scale, shift, skip

    def params(self, device):
        from mvn_rocm import v2v
        assert bool((self.w.bfloat16().float() == self.w).all())
        assert self.w.shape[0] == self.up.cin and self.w.shape[1] in self.up.couts
        return (getattr(v2v, self.up.packer)(self.w.double()).to(device), self.scale.to(device), self.shift.to(device))

    def run(self, device, x_dev=None, skip_dev=None):
        from mvn_rocm import v2v
        xd = cl(self.x, device) if x_dev is None else x_dev
        sd = skip_dev if skip_dev is not None else (cl(self.skip, device) if self.skip is not None else None)
        return getattr(v2v, self.up.fn)(xd, self.params(device), sd)

    def pre_round(self, exact=True):
        """(pre, u + skip) of the contract in float64: acc in f32 on the CPU when ``exact`` (guarded:
        the sum of |x w| is below 2^24), else in float64."""
        if exact:
            finite = torch.where(torch.isfinite(self.x), self.x, torch.zeros_like(self.x))
            assert float(F.conv_transpose3d(finite.abs(), self.w.abs(), None, stride=2).max()) < 2.0 ** 24
            acc = F.conv_transpose3d(self.x, self.w, None, stride=2).double()
        else:
            acc = F.conv_transpose3d(self.x.double(), self.w.double(), None, stride=2)
        pre = acc * per_channel(self.scale) + per_channel(self.shift)
        u = torch.where(pre <= 0, torch.zeros_like(pre), pre)
        return pre, (u + self.skip.double() if self.skip is not None else u)

    def reference(self):
        pre, r = self.pre_round()
        return r.float().bfloat16(), pre


# ----------------------------------------------------------------------------- V2VEval written out
def _front(m, vol_cl):
    """The front block and the three full-resolution blocks after it, from the public pieces."""
    from mvn_rocm import v2v
    dev = vol_cl.device
    fl = m.front_layers
    c0, b0 = fl[0].block[0], fl[0].block[1]
    h = v2v.v2v_front(vol_cl, *v2v.fold_basic3d_block(c0.weight, c0.bias, b0.weight, b0.bias, b0.running_mean,
                                                      b0.running_var, b0.eps, device=dev), torch.bfloat16)
    h = h.permute(0, 2, 3, 4, 1).contiguous()
    for i in (1, 2, 3):
        h = v2v.res3d_block(h, v2v.fold_res3d_block(fl[i], device=dev))
    return h


def chain(m, ev, vol_cl):
    """V2VEval.trunk written out from the public pieces and the stand-in's own modules."""
    from mvn_rocm import v2v
    dev = vol_cl.device
    ed = m.encoder_decoder
    h = _front(m, vol_cl)
    s1 = v2v.res3d_block(h, v2v.fold_res3d_block(ed.skip_res1, device=dev))
    x = v2v.v2v_interior(ev.interior, h.permute(0, 4, 1, 2, 3).float())
    x = (x + s1.permute(0, 4, 1, 2, 3)).permute(0, 2, 3, 4, 1).to(torch.bfloat16).contiguous()
    return v2v.res3d_block(x, v2v.fold_res3d_block(m.back_layers[0], device=dev))


def chain_kernels(m, ev, vol_cl):
    """V2VEval(half_res="kernels").trunk written out from the public functions."""
    from mvn_rocm import v2v
    dev = vol_cl.device
    ed = m.encoder_decoder
    h = _front(m, vol_cl)
    s1 = v2v.res3d_block(h, v2v.fold_res3d_block(ed.skip_res1, device=dev))
    e1 = v2v.res3d_block_wide(v2v.max_pool2_cl(h), v2v.fold_res3d_block_wide(ed.encoder_res1, device=dev))
    s2 = v2v.res3d_block_wide(e1, v2v.fold_res3d_block_wide(ed.skip_res2, device=dev))
    d = v2v.v2v_interior_deep(ev.interior, e1.permute(0, 4, 1, 2, 3).float())
    d = (d + s2.permute(0, 4, 1, 2, 3)).permute(0, 2, 3, 4, 1).to(torch.bfloat16).contiguous()
    d1 = v2v.res3d_block_wide(d, v2v.fold_res3d_block_wide(ed.decoder_res1, device=dev))
    x = v2v.upsample2_add(d1, v2v.fold_upsample_block(ed.decoder_upsample1, device=dev), s1)
    return v2v.res3d_block(x, v2v.fold_res3d_block(m.back_layers[0], device=dev))


def chain_deep(m, vol_cl):
    """V2VEval(half_res="kernels", deep="kernels").trunk written out from the public functions."""
    from mvn_rocm import v2v
    dev = vol_cl.device
    ed = m.encoder_decoder
    h = _front(m, vol_cl)

    def wide(name, x):
        return v2v.res3d_block_wide(x, v2v.fold_res3d_block_wide(getattr(ed, name), device=dev))

    def deep(name, x):
        return v2v.res3d_block_deep(x, v2v.fold_res3d_block_deep(getattr(ed, name), device=dev))

    def up(name, x, skip):
        return v2v.upsample2_add_deep(x, v2v.fold_upsample_block_deep(getattr(ed, name), device=dev), skip)

    s1 = v2v.res3d_block(h, v2v.fold_res3d_block(ed.skip_res1, device=dev))
    e1 = wide("encoder_res1", v2v.max_pool2_cl(h))
    s2 = wide("skip_res2", e1)
    x = deep("encoder_res2", v2v.max_pool2_cl(e1))
    s3 = deep("skip_res3", x)
    x = deep("encoder_res3", v2v.max_pool2_cl(x))
    s4 = deep("skip_res4", x)
    x = deep("encoder_res4", v2v.max_pool2_cl(x))
    s5 = deep("skip_res5", x)
    x = deep("mid_res", deep("encoder_res5", v2v.max_pool2_cl(x)))
    assert tuple(x.shape[1:]) == (1, 1, 1, 128) and tuple(s5.shape[1:4]) == (2, 2, 2)
    x = up("decoder_upsample5", deep("decoder_res5", x), s5)
    x = up("decoder_upsample4", deep("decoder_res4", x), s4)
    x = up("decoder_upsample3", deep("decoder_res3", x), s3)
    x = up("decoder_upsample2", deep("decoder_res2", x), s2)
    x = v2v.upsample2_add(wide("decoder_res1", x), v2v.fold_upsample_block(ed.decoder_upsample1, device=dev), s1)
    return v2v.res3d_block(x, v2v.fold_res3d_block(m.back_layers[0], device=dev))


# ----------------------------------------------------------------------------- for the API tests
def unpack_mfma_a(packed):
    """Inverse of the MFMA A-fragment layout (include/mvn_hip.h): [..., m, lane, j] holds row
    16 m + (lane & 15), K-slot 8 (lane >> 4) + j of a (rows, 32 K-slots) matrix.  (..., M, 64, 8) ->
    (..., 16 M, 32) in float64."""
    p = packed.cpu().double()
    assert p.dim() >= 3 and tuple(p.shape[-2:]) == (64, 8)
    lead, M = tuple(p.shape[:-3]), p.shape[-3]
    n = len(lead)
    a = p.reshape(*lead, M, 4, 16, 8)                            # [m][lane >> 4][lane & 15][j]
    return a.permute(*range(n), n, n + 2, n + 1, n + 3).reshape(*lead, 16 * M, 32)


def unpack_conv3(packed, co, cin=None):
    """The (co, 32 KP, 3, 3, 3) weight from a conv's packed layout [tap = (dx*3 + dy)*3 + dz][kp][m][lane][j]
    = W[16 m + (lane & 15)][32 kp + 8 (lane >> 4) + j][dx][dy][dz] (mvn_v2v_conv3 has no kp: one pass
    of 32 K-slots); with ``cin`` the shape (27, cin / 32, co / 16, 64, 8) is asserted."""
    assert cin is None or tuple(packed.shape) == (27, cin // 32, co // 16, 64, 8)
    a = unpack_mfma_a(packed)                                    # (27, [KP,] co, 32)
    if a.dim() == 3:
        a = a.unsqueeze(1)
    assert a.shape[0] == 27 and a.shape[2] == co
    return a.permute(2, 1, 3, 0).reshape(co, 32 * a.shape[1], 3, 3, 3)


def unpack_skip(packed, co, cin=None):
    """The (co, 32 KP) pointwise-skip weight from [kp][m][lane][j] (no kp: one pass); with ``cin``
    the shape is asserted, (cin / 32, co / 16, 64, 8) or (co / 16, 64, 8) for one pass."""
    want = (co // 16, 64, 8)
    assert cin is None or tuple(packed.shape) in (want, (cin // 32,) + want)
    a = unpack_mfma_a(packed)                                    # ([KP,] co, 32)
    if a.dim() == 2:
        a = a.unsqueeze(0)
    assert a.shape[1] == co
    return a.permute(1, 0, 2).reshape(co, 32 * a.shape[0])


def unpack_upsample(packed, cin, cout):
    """The (cin, cout, 2, 2, 2) ConvTranspose3d weight from an upsample's packed layout, H = cout / 16:
    [kp][m][lane][j] = W[32 kp + 8 (lane >> 4) + j][16 (m % H) + (lane & 15)][dx][dy][dz],
    (dx*2 + dy)*2 + dz = m // H."""
    H = cout // 16
    assert tuple(packed.shape) == (cin // 32, 8 * H, 64, 8)
    a = unpack_mfma_a(packed).view(cin // 32, 8, H, 16, 32)     # [kp][offset][h][row][k]
    return a.permute(0, 4, 2, 3, 1).reshape(cin, cout, 2, 2, 2)


def bn_fold64(conv, bn):
    """(scale, shift) of conv + eval-mode BatchNorm in float64."""
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
    b = conv.bias.detach().double() if conv.bias is not None else torch.zeros_like(s)
    return s, (b - bn.running_mean.double()) * s + bn.bias.detach().double()


def vol(B, V, C, dtype=torch.bfloat16):
    return torch.zeros(B, V, V, V, C, dtype=dtype)
