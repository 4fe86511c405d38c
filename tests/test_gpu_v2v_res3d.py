"""Full-resolution Res3DBlocks (csrc/v2v_res3d.hip): one 3x3x3 conv + folded BN + residual + ReLU
per launch on channels-last bf16 volumes, the one-call block, and V2VEval (MI355X only).

Most tests give the kernel operands for which its f32 arithmetic is exact in any summation
order, and compare bits (as tests/test_gpu_v2v_front_edges.py does for the front block):

* integers in [-4, 4] as inputs, weights and skip: every partial sum is an integer below
  27 * 32 * 16 = 13,824 < 2^24, so torch's f32 conv3d on the CPU is exact (guarded); ``scale`` is
  a per-channel power of two of either sign, ``shift`` a multiple of 1/4, so neither fma nor the
  residual add rounds; the only rounding left is f32 -> bf16, nearest-even, ties included;
* an impulse lattice of stride 3 with full 8-bit significands: every output receives at most
  one product (asserted), exact in f32; ``product * scale`` rounds once to f32, then to bf16.

The reference is r in float64 per the arithmetic contract of mvn_v2v_conv3 (include/mvn_hip.h),
+0 where r <= 0 (NaN kept), cast to f32, then ``.bfloat16()``; the tests assert r holds no -0.

Tiles are 4 x 8 x 16 (x, y, z); a block walks a column of V / 4 tiles along x through a ring of
6 x-slices whose slot pattern repeats every 3 tiles; the grid is B * (V / 8) * (V / 16) blocks.
Reads nothing outside the repository.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from conftest import assert_parity_with_nans

CO = 32
NONE, IDENTITY, POINTWISE = 0, 1, 2
MODES = {"none": NONE, "identity": IDENTITY, "pointwise": POINTWISE}
SKIP_C = {NONE: 0, IDENTITY: 32, POINTWISE: 16}


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


# ----------------------------------------------------------------------------- helpers
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
    """The kernel's (B, V, V, V, 32) result as (B, 32, V, V, V) on the CPU."""
    return y_cl.cpu().permute(0, 4, 1, 2, 3).contiguous()


def pack3(w, device):
    from mvn_rocm import v2v
    assert bool((w.bfloat16().float() == w).all())
    return v2v.pack_conv3_weight(w.double()).to(device)


def packs(ws, device):
    from mvn_rocm import v2v
    return v2v.pack_pointwise_skip_weight(ws.double()).to(device)


def exact_scale_shift(seed):
    """Per-channel scale = +-2^k (k in -2..1, both signs present) and shift = a multiple of 1/4
    (never -0)."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(-2, 2, (CO,), generator=g).float()
    sign = torch.where(torch.arange(CO) % 3 == 1, -1.0, 1.0)
    scale = sign * torch.exp2(k)
    shift = torch.randint(-8, 9, (CO,), generator=g).float() / 4 + 0.0
    assert not bool((torch.signbit(shift) & (shift == 0)).any())
    assert bool((scale < 0).any()) and bool((scale > 0).any())
    return scale, shift


def per_channel(t):
    return t.double().view(1, -1, 1, 1, 1)


class Case:
    """Operands of one launch on the CPU (f32 tensors holding bf16-exact values)."""

    def __init__(self, x, w, scale, shift, mode=NONE, skip=None, ws=None, scale_s=None, shift_s=None):
        self.x, self.w, self.scale, self.shift, self.mode = x, w, scale, shift, mode
        self.skip, self.ws, self.scale_s, self.shift_s = skip, ws, scale_s, shift_s

    def run(self, device, x_dev=None, skip_dev=None):
        from mvn_rocm import v2v
        xd = cl(self.x, device) if x_dev is None else x_dev
        args = [xd, pack3(self.w, device), self.scale.to(device), self.shift.to(device)]
        if self.mode != NONE:
            args.append(cl(self.skip, device) if skip_dev is None else skip_dev)
        if self.mode == POINTWISE:
            args += [packs(self.ws, device), self.scale_s.to(device), self.shift_s.to(device)]
        return v2v.v2v_conv3(*args)

    def pre_relu(self, exact=True):
        """r of the contract in float64; the conv in f32 on the CPU when ``exact`` (guarded: exact
        for these operands), else in float64."""
        x, w = self.x, self.w
        if exact:
            finite = torch.where(torch.isfinite(x), x, torch.zeros_like(x))
            assert float(F.conv3d(finite.abs(), w.abs(), None, padding=1).max()) < 2.0 ** 24
            acc = F.conv3d(x, w, None, padding=1).double()
        else:
            acc = F.conv3d(x.double(), w.double(), None, padding=1)
        r = acc * per_channel(self.scale) + per_channel(self.shift)
        if self.mode == IDENTITY:
            r = r + self.skip.double()
        elif self.mode == POINTWISE:
            w1 = self.ws.view(CO, 16, 1, 1, 1)
            acc_s = F.conv3d(self.skip, w1).double() if exact else F.conv3d(self.skip.double(), w1.double())
            r = r + (acc_s * per_channel(self.scale_s) + per_channel(self.shift_s))
        return r

    def reference(self):
        """(bf16 reference, float64 pre-relu r)."""
        r = self.pre_relu()
        assert not bool((torch.signbit(r) & (r == 0)).any()), "the pre-relu reference holds a -0"
        y = torch.where(r <= 0, torch.zeros_like(r), r)            # a NaN is neither: kept
        return y.float().bfloat16(), r


def integer_case(B, V, cin, mode, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-4, 5, (B, cin, V, V, V), generator=g).float()
    w = torch.randint(-4, 5, (CO, cin, 3, 3, 3), generator=g).float()
    scale, shift = exact_scale_shift(seed + 1)
    case = Case(x, w, scale, shift, mode)
    if mode != NONE:
        case.skip = torch.randint(-4, 5, (B, SKIP_C[mode], V, V, V), generator=g).float()
    if mode == POINTWISE:
        case.ws = torch.randint(-4, 5, (CO, 16), generator=g).float()
        case.scale_s, case.shift_s = exact_scale_shift(seed + 2)
    return case


@functools.lru_cache(maxsize=None)
def parity_case(B, V, cin, mode):
    case = integer_case(B, V, cin, mode, seed=1000 * B + V + 7 * cin + mode)
    ref, r = case.reference()
    return case, ref, r


# ----------------------------------------------------------------------------- 1. exact parity
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES.values(), ids=MODES.keys())
@pytest.mark.parametrize("cin", (16, 32))
@pytest.mark.parametrize("B,V", ((1, 16), (3, 16), (1, 32), (1, 48), (2, 48)))
def test_exact_parity_integer_inputs(device, B, V, cin, mode):
    """Every element equals the CPU reference bit for bit, every skip mode and Cin, frames of
    different data.  Grids of 2, 6, 8, 18 and 36 blocks: (1, 16) and (3, 16) have fewer blocks
    than XCDs; (3, 16), (1, 48) and (2, 48) take xcd_remap's ragged branch (6, 18, 36 are no
    multiples of 8); V = 48 has 3 z-tiles, 6 y-tiles and 12 x-tiles, so a tile with neighbours on
    both sides in every axis; the 6-slot x-slice ring repeats every 3 tiles, so V = 16 (4 tiles)
    already passes one period and V = 48 (12 tiles) four."""
    case, ref, r = parity_case(B, V, cin, mode)
    assert all(not torch.equal(case.x[0], case.x[f]) for f in range(1, B))
    finite = torch.where(torch.isfinite(case.x), case.x, torch.zeros_like(case.x))
    partial = float(F.conv3d(finite.abs(), case.w.abs(), None, padding=1).max())
    print(f"largest sum of |x w|: {partial:.0f}")
    assert partial <= 27 * cin * 16
    # what the reference must hold for the comparison to test the relu and the bf16 rounding
    pos = r[r > 0].float()
    low = bits(pos) & 0xFFFF
    assert pos.numel() >= 0.25 * r.numel()
    assert (low != 0).sum() >= 0.10 * pos.numel()               # more than 8 significant bits
    assert (low == 0x8000).any()                                # an exact tie
    y = case.run(device)
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (B, V, V, V, CO)
    assert_same_bits(ncdhw(y), ref)


# ----------------------------------------------------------------------------- 2. impulse lattice
def bf16_full(shape, g):
    """Normal bf16 values with full 8-bit significands (random normal, rounded to bf16)."""
    v = torch.randn(shape, generator=g).bfloat16().float()
    return torch.where(v.abs() > 2.0 ** -100, v, torch.ones_like(v))


def lattice_reference(x, w, scale, pad):
    """At most one product per output (asserted), so the float64 conv IS that product: times
    scale in float64, rounded once to f32 (the kernel's fma with a zero shift)."""
    k = 2 * pad + 1
    hits = F.conv3d((x != 0).double(), torch.ones(1, x.shape[1], k, k, k, dtype=torch.float64), padding=pad)
    assert float(hits.max()) == 1.0
    return (F.conv3d(x.double(), w.double(), None, padding=pad) * per_channel(scale)).float()


@pytest.mark.gpu
@pytest.mark.parametrize("cin", (16, 32))
@pytest.mark.parametrize("B,V,off", ((2, 16, 0), (2, 16, 2), (1, 48, 1)))
def test_impulse_lattice_full_mantissa(device, B, V, off, cin):
    """One product per output, 8-bit x 8-bit significands: pins the tap <-> packed-weight map,
    the channel-chunk swizzle and the border clipping one product at a time, bit for bit."""
    g = torch.Generator().manual_seed(7 * V + off + cin)
    w = (torch.randn((CO, cin, 3, 3, 3), generator=g) * 0.05).bfloat16().float()
    scale = torch.randn(CO, generator=g)
    scale[0], scale[1] = -scale[0].abs(), scale[1].abs()
    x = torch.zeros((B, cin, V, V, V))
    pts = torch.arange(off, V, 3)
    n = pts.numel()
    ch = (torch.arange(B * n ** 3).view(B, n, n, n) * 5 + 11 * torch.arange(B).view(B, 1, 1, 1)) % cin
    sub = torch.zeros(B, cin, n, n, n).scatter_(1, ch.unsqueeze(1), bf16_full((B, 1, n, n, n), g))
    x[:, :, off::3, off::3, off::3] = sub
    assert int((x != 0).sum()) == B * n ** 3 and len(set(ch.flatten().tolist())) == cin      # every channel used
    r32 = lattice_reference(x, w, scale, 1)
    ref = torch.where(r32 <= 0, torch.zeros_like(r32), r32).bfloat16()
    assert 0.2 < float((ref > 0).float().mean()) < 0.8                      # both relu branches
    y = Case(x, w, scale, torch.zeros(CO)).run(device)
    assert_same_bits(ncdhw(y), ref)


@pytest.mark.gpu
def test_impulse_pointwise_skip_weights(device):
    """The pointwise skip's packed weights one product at a time: x is zero, every skip voxel has
    one of its 16 channels set."""
    B, V = 2, 16
    g = torch.Generator().manual_seed(99)
    ws = (torch.randn((CO, 16), generator=g) * 0.3).bfloat16().float()
    scale_s = torch.randn(CO, generator=g)
    scale_s[0], scale_s[1] = -scale_s[0].abs(), scale_s[1].abs()
    ch = torch.randint(0, 16, (B, 1, V, V, V), generator=g)
    skip = torch.zeros(B, 16, V, V, V).scatter_(1, ch, bf16_full((B, 1, V, V, V), g))
    r32 = lattice_reference(skip, ws.view(CO, 16, 1, 1, 1), scale_s, 0)
    ref = torch.where(r32 <= 0, torch.zeros_like(r32), r32).bfloat16()
    assert 0.2 < float((ref > 0).float().mean()) < 0.8
    w = torch.randint(-4, 5, (CO, 32, 3, 3, 3), generator=g).float()
    case = Case(torch.zeros(B, 32, V, V, V), w, *exact_scale_shift(3)[:1], torch.zeros(CO), POINTWISE, skip, ws, scale_s,
                torch.zeros(CO))
    assert_same_bits(ncdhw(case.run(device)), ref)


# ----------------------------------------------------------------------------- 3. frames, borders
@pytest.mark.gpu
@pytest.mark.parametrize("cin,mode", ((32, IDENTITY), (16, POINTWISE), (16, NONE)), ids=("identity", "pointwise", "none16"))
def test_frames_do_not_mix(device, cin, mode):
    """In a B = 3 call each frame equals its own B = 1 call bit for bit."""
    case, ref, _ = parity_case(3, 16, cin, mode)
    xd = cl(case.x, device)
    sd = cl(case.skip, device) if mode != NONE else None
    y = case.run(device, xd, sd)
    assert_same_bits(ncdhw(y), ref)
    for f in range(3):
        alone = case.run(device, xd[f:f + 1].clone(), sd[f:f + 1].clone() if sd is not None else None)
        assert_same_bits(alone, y[f:f + 1])


@pytest.mark.gpu
@pytest.mark.parametrize("cin", (16, 32))
def test_borders_are_zero_padding(device, cin):
    """All-ones frame between two NaN frames, weights of ones, scale 1, shift 0: exactly the
    clipped tap count x Cin at faces, edges and corners — a tap that reached past the volume
    into a neighbouring frame (or anything else) would show as NaN or a wrong count."""
    V = 32
    x = torch.full((3, cin, V, V, V), float("nan"))
    x[1] = 1.0
    case = Case(x, torch.ones(CO, cin, 3, 3, 3), torch.ones(CO), torch.zeros(CO))
    y = ncdhw(case.run(device)).float()
    n = torch.full((V,), 3.0)
    n[0] = n[-1] = 2.0
    want = (n.view(V, 1, 1) * n.view(1, V, 1) * n.view(1, 1, V) * cin).expand(CO, V, V, V)
    assert set(want.unique().tolist()) == {8.0 * cin, 12.0 * cin, 18.0 * cin, 27.0 * cin}
    assert torch.equal(y[1], want)
    assert bool(torch.isnan(y[0]).all()) and bool(torch.isnan(y[2]).all())


# ----------------------------------------------------------------------------- 4. random data
def bf16r(t):
    return t.float().bfloat16().float()


def random_case(B, V, cin, mode, seed, x=None):
    g = torch.Generator().manual_seed(seed)
    if x is None:
        x = bf16r(torch.randn(B, cin, V, V, V, generator=g))
    w = bf16r(torch.randn(CO, cin, 3, 3, 3, generator=g) * (2.0 / (27 * (cin + CO))) ** 0.5 * 3)
    scale = (0.75 + 0.5 * torch.rand(CO, generator=g)) * torch.where(torch.arange(CO) % 5 == 2, -1.0, 1.0)
    shift = 0.2 * torch.randn(CO, generator=g)
    case = Case(x, w, scale, shift, mode)
    if mode != NONE:
        case.skip = bf16r(torch.randn(B, SKIP_C[mode], V, V, V, generator=g))
    if mode == POINTWISE:
        case.ws = bf16r(torch.randn(CO, 16, generator=g) * 0.2)
        case.scale_s = 0.75 + 0.5 * torch.rand(CO, generator=g)
        case.shift_s = 0.2 * torch.randn(CO, generator=g)
    return case


def check_bound(case, got, what):
    """|got - ref| <= 2^-8 |ref| + gamma S per element (half a bf16 ulp plus the worst-case f32
    summation bound), ref the float64 restatement; returns the worst fraction of the bar.  The
    same conv in f32 on the CPU must sit far inside gamma S (a bound, not a measurement)."""
    cin = case.x.shape[1]
    gamma = (27 * cin + SKIP_C[case.mode] + 4) * 2.0 ** -24
    r = case.pre_relu(exact=False)
    ref = torch.where(r <= 0, torch.zeros_like(r), r)
    S = F.conv3d(case.x.double().abs(), case.w.double().abs(), None, padding=1) * per_channel(case.scale).abs() \
        + per_channel(case.shift).abs()
    if case.mode == IDENTITY:
        S = S + case.skip.double().abs()
    elif case.mode == POINTWISE:
        S = S + F.conv3d(case.skip.double().abs(), case.ws.double().abs().view(CO, 16, 1, 1, 1)) \
            * per_channel(case.scale_s).abs() + per_channel(case.shift_s).abs()
    r32 = case.pre_relu(exact=True)                     # the f32 CPU conv (no exactness guard needed: finite data)
    cpu_frac = float(((r32 - r).abs() / (gamma * S)).max())
    bar = 2.0 ** -8 * ref.abs() + gamma * S
    frac = float(((got.double() - ref).abs() / bar).max())
    print(f"{what}: worst |got - ref| / bar = {frac:.4f}; f32 CPU conv at {cpu_frac:.4f} of gamma S")
    assert cpu_frac <= 0.05, "the f32 CPU conv is not far inside gamma S: the bar is no bound for these inputs"
    assert frac <= 1.0
    return frac


@pytest.mark.gpu
@pytest.mark.parametrize("cin,mode", ((16, POINTWISE), (32, IDENTITY)), ids=("16to32_pointwise", "32to32_identity"))
@pytest.mark.parametrize("V", (16, 32))
def test_random_data_against_float64_restatement(device, V, cin, mode):
    """conv1 (skip NONE) and conv2 (the block's skip) on random bf16 data against the float64
    restatement with the kernel's own roundings; conv2's restatement reads the hidden volume the
    GPU wrote.  Measured on the MI355X: see DESIGN.md §4.12."""
    B = 2
    c1 = random_case(B, V, cin, NONE, seed=10 * V + cin)
    xd = cl(c1.x, device)
    h = c1.run(device, xd)
    check_bound(c1, ncdhw(h).float(), f"conv1 V={V} cin={cin}")
    c2 = random_case(B, V, 32, mode, seed=10 * V + cin + 1, x=ncdhw(h).float())
    c2.skip = c1.x
    y = c2.run(device, h, xd)
    check_bound(c2, ncdhw(y).float(), f"conv2 V={V} {('none', 'identity', 'pointwise')[mode]}")


# ----------------------------------------------------------------------------- 5. non-finite voxels
# 3^3 boxes pairwise disjoint: both corners, either side of the x seam 11 | 12, of the y seam
# 7 | 8 and of the z seam 15 | 16 (tiles are 4 x 8 x 16)
NAN_VOXELS = ((0, 0, 0), (31, 31, 31), (11, 20, 5), (12, 20, 27), (24, 7, 8), (24, 8, 24), (20, 27, 15), (4, 27, 16))
INF_VOXELS = ((12, 12, 12, 5, float("inf")), (22, 20, 7, 13, float("-inf")))      # x, y, z, channel, value
N_BOX = 2 * 2 ** 3 + 6 * 3 ** 3


def box_mask(V, voxels, pad):
    m = np.zeros((V, V, V), bool)
    for x, y, z in voxels:
        m[max(x - pad, 0):x + pad + 1, max(y - pad, 0):y + pad + 1, max(z - pad, 0):z + pad + 1] = True
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("cin", (16, 32))
def test_nonfinite_input_voxels_follow_torch(device, cin):
    """A NaN input voxel is NaN in exactly its clipped 3^3 box, all 32 channels; +-inf voxels
    (positive weights, scales of both signs) come out +inf or 0; every other element is
    bit-equal, and the clean frame equals its run alone."""
    V = 32
    case = integer_case(3, V, cin, NONE, seed=77 + cin)
    for n, (px, py, pz) in enumerate(NAN_VOXELS):
        case.x[0, (5 * n + 2) % cin, px, py, pz] = float("nan")
    g = torch.Generator().manual_seed(78)
    for px, py, pz, ch, val in INF_VOXELS:
        case.x[2, ch, px, py, pz] = val
        case.w[:, ch] = torch.randint(1, 5, (CO, 3, 3, 3), generator=g).float()       # no 0 * inf
    ref, _ = case.reference()
    ref = ref.float()
    nan_ref = torch.isnan(ref).numpy()
    box = box_mask(V, NAN_VOXELS, 1)
    assert box.sum() == N_BOX                                     # pairwise disjoint boxes
    assert (nan_ref[0] == box[None]).all() and not nan_ref[1:].any()
    inf_ref = torch.isinf(ref).numpy()
    assert not inf_ref[:2].any() and inf_ref[2].any() and bool((ref[torch.isinf(ref)] > 0).all())
    for (px, py, pz, _, val) in INF_VOXELS:
        at = ref[2, :, px, py, pz]
        assert bool((torch.isinf(at) == ((case.scale > 0) == (val > 0))).all()) and bool((at[~torch.isinf(at)] == 0).all())
    xd = cl(case.x, device)
    y = case.run(device, xd)
    assert_parity_with_nans(ncdhw(y).float().numpy(), ref.numpy(), "sum")
    assert int(torch.isnan(y).sum()) == CO * N_BOX
    assert_same_bits(case.run(device, xd[1:2].clone()), y[1:2])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (IDENTITY, POINTWISE), ids=("identity", "pointwise"))
def test_nonfinite_skip_voxels_reach_their_own_voxel(device, mode):
    """Under an IDENTITY / POINTWISE skip a non-finite skip voxel reaches exactly its own voxel."""
    V = 32
    case = integer_case(3, V, 32, mode, seed=91 + mode)
    sc = SKIP_C[mode]
    for n, (px, py, pz) in enumerate(NAN_VOXELS):
        case.skip[0, (5 * n + 2) % sc, px, py, pz] = float("nan")
    for px, py, pz, ch, val in INF_VOXELS:
        case.skip[2, ch, px, py, pz] = val
    if mode == POINTWISE:
        g = torch.Generator().manual_seed(92)
        for *_, ch, _ in INF_VOXELS:
            case.ws[:, ch] = torch.randint(1, 5, (CO,), generator=g).float()           # no 0 * inf
    ref, _ = case.reference()
    ref = ref.float()
    nan_ref = torch.isnan(ref).numpy()
    own = box_mask(V, NAN_VOXELS, 0)
    if mode == IDENTITY:          # the NaN sits in one channel of the 32 and stays there
        assert int(nan_ref.sum()) == len(NAN_VOXELS) and not nan_ref[1:].any()
    else:                         # the 1x1x1 conv spreads it over all 32 channels of the voxel
        assert (nan_ref[0] == own[None]).all() and not nan_ref[1:].any()
    assert not torch.isinf(ref[:2]).any() and torch.isinf(ref[2]).any()
    # identity: only the +inf voxel stays infinite (-inf is below the relu); pointwise: both, in
    # the channels whose scale has the matching sign
    assert int(torch.isinf(ref).any(dim=1).sum()) == (1 if mode == IDENTITY else len(INF_VOXELS))
    xd, sd = cl(case.x, device), cl(case.skip, device)
    y = case.run(device, xd, sd)
    assert_parity_with_nans(ncdhw(y).float().numpy(), ref.numpy(), "sum")
    assert_same_bits(case.run(device, xd[1:2].clone(), sd[1:2].clone()), y[1:2])


# ----------------------------------------------------------------------------- 6. stray reads, writes
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


@pytest.mark.gpu
@pytest.mark.parametrize("cin,mode", ((32, IDENTITY), (16, POINTWISE)), ids=("identity", "pointwise"))
def test_no_reads_or_writes_outside_the_tensors(device, cin, mode):
    """The C entries on slices of larger buffers (V = 16, B = 2: every tile touches the border):
    the NaN bands around x and skip must not reach the result, and the sentinel bands around the
    output and around the workspace (passed at exactly its advertised size) must be intact, with
    no sentinel left inside the output."""
    from mvn_rocm import _lib, v2v
    from mvn_rocm._ops import _stream
    lib = _lib.load()
    B, V = 2, 16
    # one launch
    case, ref, _ = parity_case(3, V, 32, mode)
    big_x, xin = banded(cl(case.x[:B], device))
    big_s, sin = banded(cl(case.skip[:B], device))
    big_o, out = banded(((B, V, V, V, CO), device))
    w, sc, sh = pack3(case.w, device), case.scale.to(device), case.shift.to(device)
    pw = [packs(case.ws, device), case.scale_s.to(device), case.shift_s.to(device)] if mode == POINTWISE else [None] * 3
    assert xin.data_ptr() % 16 == 0 and sin.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    code = lib.mvn_v2v_conv3(xin.data_ptr(), 32, w.data_ptr(), sc.data_ptr(), sh.data_ptr(), mode, sin.data_ptr(),
                             SKIP_C[mode], *[t.data_ptr() if t is not None else None for t in pw], out.data_ptr(), B, V,
                             _stream(xin))
    _lib.check(code, "mvn_v2v_conv3")
    torch.cuda.synchronize()
    assert bands_intact(big_o, out.numel(), True)
    assert_same_bits(ncdhw(out), ref[:B])
    for big, n in ((big_x, xin.numel()), (big_s, sin.numel())):
        assert bool(torch.isnan(big[:BAND]).all()) and bool(torch.isnan(big[BAND + n:]).all())
    # the one-call block: cin -> 32 with the block's own skip
    params = v2v.fold_res3d_block(randomise(Res3DBlock(cin, CO), 5), device=device)
    x = bf16r(torch.randn(3, cin, V, V, V, generator=torch.Generator().manual_seed(6)))
    big_x, xin = banded(cl(x, device))
    big_o, out = banded(((3, V, V, V, CO), device))
    ws_bytes = lib.mvn_v2v_res3d_workspace_bytes(2, V)
    assert ws_bytes == 2 * V ** 3 * CO * 2
    big_w, ws = banded(((ws_bytes // 2,), device))
    ptr = [t.data_ptr() if t is not None else None for t in params]
    code = lib.mvn_v2v_res3d(xin.data_ptr(), cin, *ptr[:6], IDENTITY if cin == 32 else POINTWISE, *ptr[6:],
                             out.data_ptr(), ws.data_ptr(), ws_bytes, 2, 3, V, _stream(xin))
    _lib.check(code, "mvn_v2v_res3d")
    torch.cuda.synchronize()
    assert bands_intact(big_o, out.numel(), True) and bands_intact(big_w, ws.numel(), False)
    assert bool(torch.isnan(big_x[:BAND]).all()) and bool(torch.isnan(big_x[BAND + xin.numel():]).all())
    assert_same_bits(out, v2v.res3d_block(cl(x, device), params, 2))
    assert not bool(torch.isnan(out).any())


# ----------------------------------------------------------------------------- 7. V = 256
PERIOD = 11           # coprime to every power of two: an address off by 2^k voxels changes the data


def periodic_map(V, S):
    """Index into the S^3 conv of the same periodic pattern that equals output q of the V^3 conv
    (V = S mod 11, S >= 15): the 2 voxels at either border keep their distance to it, the
    interior (no border within 1 voxel of the window) repeats with the period."""
    q = np.arange(V)
    return np.where(q < 2, q, np.where(q >= V - 2, S - (V - q), 2 + (q - 2) % PERIOD))


def periodic_volume(pat, V):
    i = torch.arange(V) % PERIOD
    return pat[:, i][:, :, i][:, :, :, i].unsqueeze(0)


def test_periodic_map_on_the_cpu():
    """The index map of the V = 256 test, at V = 32 against a direct conv (no GPU)."""
    V, S = 32, 21
    assert V % PERIOD == S % PERIOD and S >= 15
    g = torch.Generator().manual_seed(256)
    pat = torch.randint(-4, 5, (32, PERIOD, PERIOD, PERIOD), generator=g).float()
    w = torch.randint(-4, 5, (CO, 32, 3, 3, 3), generator=g).float()
    scale, shift = exact_scale_shift(256)
    full, _ = Case(periodic_volume(pat, V), w, scale, shift).reference()
    small, _ = Case(periodic_volume(pat, S), w, scale, shift).reference()
    m = torch.from_numpy(periodic_map(V, S))
    assert_same_bits(full, small[:, :, m][:, :, :, m][:, :, :, :, m])


@pytest.mark.gpu
def test_v256_whole_volume(device):
    """The largest volume the entry takes (512 blocks of 64 tiles; (gy * V + gz) * 4 + c fills
    the staging descriptor's 18 bits, gx * V * V * 64 reaches 2^30), every element checked: the
    input repeats an integer pattern with period 11 per axis, so the reference is a 25^3 CPU conv
    expanded through periodic_map (asserted on the CPU above).  About 3 GiB on the device."""
    from mvn_rocm import v2v
    V, S = 256, 25
    assert V % PERIOD == S % PERIOD and S >= 15
    g = torch.Generator().manual_seed(256)
    pat = torch.randint(-4, 5, (32, PERIOD, PERIOD, PERIOD), generator=g).float()
    w = torch.randint(-4, 5, (CO, 32, 3, 3, 3), generator=g).float()
    scale, shift = exact_scale_shift(256)
    ref_s, _ = Case(periodic_volume(pat, S), w, scale, shift).reference()
    assert float((ref_s > 0).float().mean()) > 0.25
    i = (torch.arange(V) % PERIOD).to(device)
    pcl = pat.bfloat16().permute(1, 2, 3, 0).contiguous().to(device)
    x = pcl.index_select(0, i).index_select(1, i).index_select(2, i).unsqueeze(0)
    assert tuple(x.shape) == (1, V, V, V, 32) and x.is_contiguous()
    y = v2v.v2v_conv3(x, pack3(w, device), scale.to(device), shift.to(device))
    del x
    m = torch.from_numpy(periodic_map(V, S)).to(device)
    ref = ref_s.permute(0, 2, 3, 4, 1).contiguous().to(device).index_select(1, m).index_select(2, m).index_select(3, m)
    assert y.shape == ref.shape
    same = torch.equal(y.view(torch.int16), ref.view(torch.int16))
    nbad = 0 if same else int((y.view(torch.int16) != ref.view(torch.int16)).sum())
    del y, ref
    torch.cuda.empty_cache()
    assert same, f"{nbad} elements differ in their bits"


# ----------------------------------------------------------------------------- 8. one-call block
@pytest.mark.gpu
@pytest.mark.parametrize("cin", (16, 32), ids=("16to32_pointwise", "32to32_identity"))
def test_one_call_block_equals_the_two_launches(device, cin):
    """res3d_block for group_frames 0, 1 and 2 (ragged) at B = 3 equals conv1 (skip NONE) then
    conv2 (the block's skip) on the whole batch bit for bit; Res3DBlockCL.from_reference of a
    stand-in block with non-trivial BN statistics and conv biases equals res3d_block with the
    folded parameters, and stays near the stock block in f32."""
    from mvn_rocm import v2v
    B, V = 3, 16
    block = randomise(Res3DBlock(cin, CO), seed=40 + cin)
    p = v2v.fold_res3d_block(block, device=device)
    assert (p.skip_packed is None) == (cin == 32)
    x = bf16r(torch.randn(B, cin, V, V, V, generator=torch.Generator().manual_seed(cin)))
    xd = cl(x, device)
    h = v2v.v2v_conv3(xd, p.packed1, p.scale1, p.shift1)
    two = v2v.v2v_conv3(h, p.packed2, p.scale2, p.shift2, xd, p.skip_packed, p.skip_scale, p.skip_shift)
    for gf in (0, 1, 2):
        assert_same_bits(v2v.res3d_block(xd, p, gf), two)
    mod = v2v.Res3DBlockCL.from_reference(block, device=device)
    assert_same_bits(mod(xd), two)
    with torch.no_grad():
        stock = block(x)
    err = float((ncdhw(two).float() - stock).abs().max() / stock.abs().max())
    print(f"block against the stock f32 modules: {err:.3e} of max|ref|")
    assert err <= 2.0 ** -6                 # two bf16 roundings deep (weights, hidden volume, output)


@pytest.mark.gpu
def test_empty_batch_and_noncontiguous_input(device):
    """An empty batch returns the empty volume without a launch; a non-contiguous view is copied."""
    from mvn_rocm import v2v
    case, ref, _ = parity_case(1, 16, 32, IDENTITY)
    p = v2v.fold_res3d_block(randomise(Res3DBlock(32, CO), 1), device=device)
    empty = torch.zeros((0, 16, 16, 16, 32), dtype=torch.bfloat16, device=device)
    c1 = (p.packed1, p.scale1, p.shift1)
    for y in (v2v.v2v_conv3(empty, *c1), v2v.v2v_conv3(empty, *c1, empty), v2v.res3d_block(empty, p)):
        assert tuple(y.shape) == (0, 16, 16, 16, 32) and y.dtype == torch.bfloat16
    view = case.x.bfloat16().to(device).permute(0, 2, 3, 4, 1)            # NCDHW storage
    sview = case.skip.bfloat16().to(device).permute(0, 2, 3, 4, 1)
    assert not view.is_contiguous()
    assert_same_bits(ncdhw(case.run(device, view, sview)), ref)


# ----------------------------------------------------------------------------- 9, 10. V2VEval
J = 17


@functools.lru_cache(maxsize=None)
def stand_in_model():
    return randomise(V2VModel(32, J), seed=2024, bias=0.02)


def chain(m, ev, vol_cl):
    """V2VEval.trunk written out from the public pieces and the stand-in's own modules."""
    from mvn_rocm import v2v
    dev = vol_cl.device
    fl, ed = m.front_layers, m.encoder_decoder
    h = v2v.v2v_front(vol_cl, *v2v.fold_basic3d_block(fl[0].block[0].weight, fl[0].block[0].bias, fl[0].block[1].weight,
                                                      fl[0].block[1].bias, fl[0].block[1].running_mean,
                                                      fl[0].block[1].running_var, fl[0].block[1].eps, device=dev),
                      torch.bfloat16)
    h = h.permute(0, 2, 3, 4, 1).contiguous()
    for i in (1, 2, 3):
        h = v2v.res3d_block(h, v2v.fold_res3d_block(fl[i], device=dev))
    s1 = v2v.res3d_block(h, v2v.fold_res3d_block(ed.skip_res1, device=dev))
    x = v2v.v2v_interior(ev.interior, h.permute(0, 4, 1, 2, 3).float())
    x = (x + s1.permute(0, 4, 1, 2, 3)).permute(0, 2, 3, 4, 1).to(torch.bfloat16).contiguous()
    return v2v.res3d_block(x, v2v.fold_res3d_block(m.back_layers[0], device=dev))


@pytest.mark.gpu
def test_v2veval_wiring(device):
    """trunk and forward equal, bit for bit, the same chain written out here (V = 32, B = 2); the
    interior runs the stand-in's own modules (V2VEval's copy of them: the same parameters)."""
    from mvn_rocm import v2v, volumetric
    import copy
    B, V = 2, 32
    m = stand_in_model()
    ev = v2v.V2VEval.from_reference(m, device=device)
    md = copy.deepcopy(m).to(device)
    own = [p for n, p in md.encoder_decoder.named_parameters() if not n.startswith("skip_res1.")]
    mine = list(ev.interior.parameters())
    assert len(mine) == len(own) and all(torch.equal(a, b) for a, b in zip(mine, own))
    vol = bf16r(torch.randn(B, V, V, V, 32, generator=torch.Generator().manual_seed(9))).bfloat16().to(device)
    coords = volumetric.build_coord_volumes(np.array([[10.0, -20.0, 900.0], [-150.0, 40.0, 1000.0]]), 2500.0, V,
                                            theta=[0.0, 0.7], device=device)
    with torch.no_grad():
        want = chain(m, ev, vol)
        got = ev.trunk(vol)
        assert got.dtype == torch.bfloat16 and tuple(got.shape) == (B, V, V, V, 32)
        assert_same_bits(got, want)
        kp, out = ev(vol, coords, 3.0)
        kp_w, out_w = v2v.v2v_head_softargmax(want, *v2v.fold_v2v_head(m.back_layers[1], m.back_layers[2], m.output_layer,
                                                                       device=device),
                                              coords, multiplier=3.0, channels_last=True)
    assert tuple(kp.shape) == (B, J, 3) and tuple(out.shape) == (B, J, V, V, V)
    assert_same_bits(kp, kp_w)
    assert_same_bits(out, out_w)


def bf16_operand_model(m):
    """The stand-in on the CPU with every conv operand rounded to bf16: weights rounded once, the
    input of every Conv3d / ConvTranspose3d rounded by a forward pre-hook; everything else f32."""
    import copy
    mb = copy.deepcopy(m)
    with torch.no_grad():
        for mod in mb.modules():
            if isinstance(mod, (nn.Conv3d, nn.ConvTranspose3d)):
                mod.weight.copy_(bf16r(mod.weight))
                mod.register_forward_pre_hook(lambda _m, args: (bf16r(args[0]),))
    return mb


E2E_SIDE = 2500.0
E2E_MULT = 10.0
# measured on the MI355X (see test_v2veval_against_the_f32_modules): the bars are twice these
E2E_TRUNK_MEASURED = 6.630e-3
E2E_JOINTS_MEASURED = 5.979e-3


def e2e_case(device):
    """Blob-like input (synth.blob_volumes in the first 17 of 32 channels, unit noise elsewhere)
    and a multiplier that makes the stand-in's logits peaked."""
    from mvn_rocm import synth, volumetric
    V = 32
    coords = volumetric.build_coord_volumes(np.array([[10.0, -20.0, 900.0]]), E2E_SIDE, V, theta=[0.3], device=device)
    blobs = synth.blob_volumes(coords, J, seed=4).cpu()
    x = torch.cat([blobs, 0.1 * torch.randn(1, 32 - J, V, V, V, generator=torch.Generator().manual_seed(2))], dim=1)
    return bf16r(x), coords


def e2e_measure(device, mult=None):
    """(trunk error / max|ref|, joints error / cuboid side) of V2VEval and of the bf16-operand CPU
    stand-in, both against the f32 stand-in on the CPU followed by torch's soft-argmax."""
    from mvn_rocm import v2v
    from oracle import restate_torch
    mult = E2E_MULT if mult is None else mult
    m = stand_in_model()
    x, coords = e2e_case(device)
    cc = coords.cpu()
    with torch.no_grad():
        def cpu(model):
            t = model.back_layers[0](model.encoder_decoder(model.front_layers(x)))
            logits = model.output_layer(model.back_layers[2](model.back_layers[1](t)))
            kp, _ = restate_torch.integrate_tensor_3d_with_coordinates(logits * mult, cc, softmax=True)
            return t, kp, logits
        t_ref, kp_ref, logits = cpu(m)
        t_b, kp_b, _ = cpu(bf16_operand_model(m))
        ev = v2v.V2VEval.from_reference(m, device=device)
        vol = x.bfloat16().permute(0, 2, 3, 4, 1).contiguous().to(device)
        t = ncdhw(ev.trunk(vol)).float()
        kp, _ = ev(vol, coords, mult)
    peak = float(((logits * mult).amax(dim=(2, 3, 4)) - (logits * mult).mean(dim=(2, 3, 4))).min())
    den = float(t_ref.abs().max())
    res = dict(peak=peak,
               trunk=float((t - t_ref).abs().max()) / den, joints=float((kp.cpu() - kp_ref).abs().max()) / E2E_SIDE,
               trunk_bf16_cpu=float((t_b - t_ref).abs().max()) / den,
               joints_bf16_cpu=float((kp_b - kp_ref).abs().max()) / E2E_SIDE)
    print("V2VEval against the f32 stand-in: " + ", ".join(f"{k} {v:.3e}" for k, v in res.items()))
    return res


@pytest.mark.gpu
def test_v2veval_against_the_f32_modules(device):
    """The true semantics: the stand-in V2VModel (Xavier weights, randomised BN statistics) in f32
    on the CPU followed by torch's soft-argmax (oracle/restate_torch.py), against V2VEval on the
    GPU at V = 32, B = 1.  Input: synth.blob_volumes (peak 10, sigma 3 voxels, unit noise) in the
    first 17 of the 32 channels, 0.1 x unit noise in the rest, rounded to bf16; multiplier 10, which
    puts every joint's largest logit 10.2 or more above its mean (the height of the blobs).
    Measured on the MI355X: trunk max error 6.630e-3 of max|ref|, joints 5.979e-3 of the 2500 mm
    cuboid side (14.9 mm).  The same stand-in on the CPU with every conv operand rounded to bf16
    (bf16_operand_model), the cost of bf16 operands alone: trunk 4.179e-3, joints 9.090e-3 — the
    joints match it (0.66 x), the trunk is 1.59 x above it (V2VEval also rounds each block's
    output, the skip it re-reads and the front block's output to bf16).  With multiplier 40 (peaks
    41 above the mean, a near-argmax) both are 4 % of the side: 3.978e-2 against 3.725e-2.  The
    bars are twice the measured values, the margin of test_end_to_end_against_the_f32_modules."""
    res = e2e_measure(device)
    assert res["peak"] > 4.0                          # peaked logits: each joint's peak well above its mean
    assert res["trunk"] <= 2 * E2E_TRUNK_MEASURED
    assert res["joints"] <= 2 * E2E_JOINTS_MEASURED
