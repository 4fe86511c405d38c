"""What the deconv-head tests share (tests/test_deconv_head_api.py, test_gpu_deconv_head.py,
test_gpu_backbone_eval.py): the operands of one mvn_deconv4s2 launch on the CPU, the arithmetic
contract of include/mvn_hip.h restated with F.conv_transpose2d (f32 where the sums are exact, float64
otherwise), the contract's error bound, the unpacker by the documented layout and the 2-D variant of
``v2v_kit.randomise``.  Nothing here is read from the code under test.  Not a test module and not a
conftest.  Reads nothing outside the repository.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from v2v_kit import BAND, SENTINEL, bf16r, exact_scale_shift, unpack_mfma_a

COUT = 256
# (M, Cin, H, W): one pixel; odd sizes below a tile; more than one row tile (4 rows); the first real
# layer's map; the largest Cin (64 K-chunks); one tile row of the last layer (3 column tiles of 16)
SHAPES = ((2, 32, 1, 1), (2, 32, 3, 5), (1, 64, 5, 7), (2, 256, 12, 12), (1, 2048, 4, 3), (1, 256, 48, 8))
SMALL = SHAPES[:5]


def shape_id(s):
    return "x".join(map(str, s))


def cl2d(x, device):
    """(M, C, H, W) f32 holding bf16-exact values (or non-finite ones) -> the kernel's (M, H, W, C) bf16."""
    xb = x.bfloat16()
    assert bool(((xb.float() == x) | torch.isnan(x)).all()), "the test's input is not exact in bf16"
    return xb.permute(0, 2, 3, 1).contiguous().to(device)


def nchw(y_cl):
    """The kernel's (M, 2H, 2W, C) result as (M, C, 2H, 2W) on the CPU."""
    return y_cl.cpu().permute(0, 3, 1, 2).contiguous()


def per_channel(t):
    return t.double().view(1, -1, 1, 1)


def deconv(x, w):
    return F.conv_transpose2d(x, w, None, stride=2, padding=1)


class DeconvCase:
    """Operands of one launch on the CPU: x (M, Cin, H, W), w (Cin, 256, 4, 4) f32 tensors of bf16-exact
    values, scale and shift (256,) f32."""

    def __init__(self, x, w, scale, shift):
        assert w.shape[0] == x.shape[1] and tuple(w.shape[1:]) == (COUT, 4, 4)
        self.x, self.w, self.scale, self.shift = x, w, scale, shift

    def params(self, device):
        from mvn_rocm import backbone
        assert bool((self.w.bfloat16().float() == self.w).all())
        return (backbone.pack_deconv4_weight(self.w.double()).to(device), self.scale.to(device), self.shift.to(device))

    def run(self, device, layout="cl", dtype=None, x_dev=None):
        from mvn_rocm import backbone
        xd = cl2d(self.x, device) if x_dev is None else x_dev
        return backbone.deconv4s2(xd, self.params(device), layout, dtype)

    def abs_sum(self):
        """The largest sum of |x w| over an output, non-finite pixels left out."""
        finite = torch.where(torch.isfinite(self.x), self.x, torch.zeros_like(self.x))
        return float(deconv(finite.abs(), self.w.abs()).max())

    def pre_relu(self, exact=True):
        """r of the contract in float64; the deconv in f32 on the CPU when ``exact`` (guarded: the sum of
        |x w| is below 2^24, so no order of accumulation rounds), else in float64."""
        if exact:
            assert self.abs_sum() < 2.0 ** 24
            acc = deconv(self.x, self.w).double()
        else:
            acc = deconv(self.x.double(), self.w.double())
        return acc * per_channel(self.scale) + per_channel(self.shift)

    def reference(self):
        """(f32 reference (M, 256, 2H, 2W), float64 pre-relu r): +0 where r <= 0, a NaN kept."""
        r = self.pre_relu()
        assert not bool((torch.signbit(r) & (r == 0)).any()), "the pre-relu reference holds a -0"
        y = torch.where(r <= 0, torch.zeros_like(r), r)            # a NaN is neither: kept
        y32 = y.float()
        assert bool(((y32.double() == y) | torch.isnan(y)).all()), "the reference is not exact in f32"
        return y32, r


def integer_case(shape, seed):
    """Integers in [-4, 4], scale +-2^k, shift in quarters: every sum is exact in f32 in any order."""
    M, cin, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-4, 5, (M, cin, H, W), generator=g).float()
    w = torch.randint(-4, 5, (cin, COUT, 4, 4), generator=g).float()
    return DeconvCase(x, w, *exact_scale_shift(seed + 1, COUT))


@functools.lru_cache(maxsize=None)
def parity_case(shape):
    """The integer case of a shape and its reference, computed once and shared (read-only)."""
    case = integer_case(shape, seed=1000 * shape[0] + shape[1] + 7 * shape[2] + 13 * shape[3])
    ref, r = case.reference()
    return case, ref, r


def random_case(shape, seed):
    """randn inputs, weights of std 3 sqrt(2 / (16 (Cin + 256))), scale in [0.75, 1.25] of both signs."""
    M, cin, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = bf16r(torch.randn(M, cin, H, W, generator=g))
    w = bf16r(torch.randn(cin, COUT, 4, 4, generator=g) * (2.0 / (16 * (cin + COUT))) ** 0.5 * 3)
    scale = (0.75 + 0.5 * torch.rand(COUT, generator=g)) * torch.where(torch.arange(COUT) % 5 == 2, -1.0, 1.0)
    return DeconvCase(x, w, scale, 0.2 * torch.randn(COUT, generator=g))


def gamma_S(case):
    """(gamma, S, float64 pre-relu r) of the contract's bound: gamma = (4 Cin + 4) 2^-24, the worst-case
    f32 summation bound of the 4 Cin products, the fma and the final rounding; S the sum of the
    absolute terms."""
    cin = case.x.shape[1]
    gamma = (4 * cin + 4) * 2.0 ** -24
    S = deconv(case.x.double().abs(), case.w.double().abs()) * per_channel(case.scale).abs() + per_channel(case.shift).abs()
    return gamma, S, case.pre_relu(exact=False)


def check_bound(case, got, what, f32_out=False):
    """|got - ref| <= 2^-8 |ref| + gamma S per element (half a bf16 ulp plus the summation bound; the
    2^-8 term dropped for an f32 output), ref the float64 restatement; returns the worst fraction of
    the bar.  The same deconv in f32 on the CPU must sit far inside gamma S (a bound, not a
    measurement)."""
    gamma, S, r = gamma_S(case)
    ref = torch.where(r <= 0, torch.zeros_like(r), r)
    r32 = deconv(case.x, case.w).double() * per_channel(case.scale) + per_channel(case.shift)
    cpu_frac = float(((r32 - r).abs() / (gamma * S)).max())
    bar = gamma * S if f32_out else 2.0 ** -8 * ref.abs() + gamma * S
    frac = float(((got.double() - ref).abs() / bar).max())
    print(f"{what}: worst |got - ref| / bar = {frac:.4f}; f32 CPU deconv at {cpu_frac:.4f} of gamma S")
    assert cpu_frac <= 0.05, "the f32 CPU deconv is not far inside gamma S: the bar is no bound for these inputs"
    assert frac <= 1.0
    return frac


def index_weight(cin):
    """A bf16-exact weight that encodes its own index: the exponent holds the tap and ci % 8 (the slot
    within a lane's 8 K-values), the significand and the sign hold co mixed with ci // 8 (the lane
    group and the K-chunk).  Two slots that a wrong read could confuse differ in value."""
    ci = torch.arange(cin).view(cin, 1, 1, 1)
    co = torch.arange(COUT).view(1, COUT, 1, 1)
    tap = (torch.arange(4).view(4, 1) * 4 + torch.arange(4).view(1, 4)).view(1, 1, 4, 4)
    mant = ((co % 128) * 37 + (ci // 8) * 53) % 128
    sign = torch.where(co >= 128, -1.0, 1.0)
    w = sign * (1.0 + mant.double() / 128) * torch.exp2((tap * 8 + ci % 8 - 64).double())
    w = w.float().expand(cin, COUT, 4, 4).contiguous()
    assert bool((w.bfloat16().float() == w).all())
    return w


def unpack_deconv4(packed, cin):
    """The (cin, 256, 4, 4) weight from the documented layout (include/mvn_hip.h):
    [tap = ky*4 + kx][kp][m][lane][j] = W[32 kp + 8 (lane >> 4) + j][16 m + (lane & 15)][ky][kx]."""
    assert tuple(packed.shape) == (16, cin // 32, COUT // 16, 64, 8) and packed.dtype == torch.bfloat16
    a = unpack_mfma_a(packed)                                    # (16, KP, 256 rows = co, 32 K-slots = ci % 32)
    return a.permute(1, 3, 2, 0).reshape(cin, COUT, 4, 4)


def unpack_by_loops(packed, cin, picks):
    """The documented element formula read literally, for a few (tap, kp, m, lane, j)."""
    out = []
    for tap, kp, m, lane, j in picks:
        out.append(((32 * kp + 8 * (lane >> 4) + j, 16 * m + (lane & 15), tap // 4, tap % 4),
                    float(packed[tap, kp, m, lane, j])))
    return out


def randomise2d(module, seed, bias=0.1):
    """``v2v_kit.randomise`` for 2-D layers: Xavier-normal conv weights, small biases, BatchNorm
    statistics of a trained layer's order of magnitude; eval mode."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
                rf = m.weight[0, 0].numel()
                fan = (m.weight.shape[0] + m.weight.shape[1]) * rf
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan) ** 0.5)
                if m.bias is not None:
                    m.bias.copy_(torch.randn(m.bias.shape, generator=g) * bias)
            elif isinstance(m, nn.BatchNorm2d):
                n = m.num_features
                m.weight.copy_(0.75 + 0.5 * torch.rand(n, generator=g))
                m.bias.copy_(0.2 * torch.randn(n, generator=g))
                if m.running_mean is not None:
                    m.running_mean.copy_(0.2 * torch.randn(n, generator=g))
                    m.running_var.copy_(0.75 + 0.5 * torch.rand(n, generator=g))
    return module.eval()


SENTINEL_F32 = 0x7FA5A5A5    # a NaN with its own payload


def banded_out(shape, dtype, device):
    """(the larger buffer as integers, the view of ``shape`` inside it, the sentinel): sentinel bands
    of 64 KiB and a sentinel fill, for a bf16 or f32 output."""
    n = int(np.prod(shape))
    if dtype == torch.bfloat16:
        big = torch.full((BAND + n + BAND,), SENTINEL, dtype=torch.int16, device=device)
        return big, big[BAND:BAND + n].view(torch.bfloat16).view(shape), SENTINEL
    s = int(np.array(SENTINEL_F32, np.uint32).view(np.int32))
    big = torch.full((BAND + n + BAND,), s, dtype=torch.int32, device=device)
    return big, big[BAND:BAND + n].view(torch.float32).view(shape), s
