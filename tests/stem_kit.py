"""What the tests of the ResNet stem's kernel share (tests/test_stem_api.py, test_gpu_stem.py,
test_gpu_stem_trunk.py): the operands of one mvn_stem launch on the CPU, the arithmetic contract of
include/mvn_hip.h restated with F.conv2d and F.max_pool2d (f32 where the sums are exact, float64 otherwise),
the contract's error bound, an index weight, and the unpacker by the documented layout.  Nothing here is read
from the code under test.  Not a test module and not a conftest.  Reads nothing outside the repository.

The kernel's tiles, restated: a block takes TILE x TILE = 8 x 8 pooled pixels of one image in all 64 channels,
so the block seams lie between pooled rows (and columns) 8 k - 1 | 8 k.  The 17 x 17 convolution pixels under
a tile (rows 16 t - 1 .. 16 t + 15 of the map for tile row t, the same in x) are numbered flat, p = 17 row +
column, and taken 16 at a time: the fragment seams are at p = 16 k - 1 | 16 k for k = 1 .. 18, and fragment f
goes to wave f % 4, so every fragment seam is a wave seam as well.  Along the channels a lane holds 4, an
accumulator 16 and a pool thread 8.  The K axis has 24 slots per tap row, 21 of them real.
"""
import functools

import torch
import torch.nn.functional as F

from bottleneck_kit import relu64, shape_id  # noqa: F401  (re-exported)
from v2v_kit import bf16r, exact_scale_shift, unpack_mfma_a

TILE, CONV_TILE, FRAG_PIX, WAVES = 8, 17, 16, 4
COUT, CIN, KS, K_REAL, ROW_SLOTS, K_SLOTS = 64, 3, 7, 147, 24, 192

# (M, H, W)
SEAM_SHAPE = (2, 35, 34)        # Hc x Wc = 18 x 17, Hp x Wp = 9 x 9: TILE + 1 pooled pixels along each axis, so the
                                # first tile is whole (all 19 fragments, every fragment and wave seam) and the
                                # block seam 7 | 8 is crossed both ways
INTERIOR_SHAPE = (1, 67, 70)    # 17 x 18 pooled pixels, 3 x 3 tiles: the middle one has neighbours on every side
SHAPES = (
    (1, 1, 1),                  # a single output: every tap but the centre is outside the image
    (2, 2, 3),
    (1, 7, 9),
    (3, 40, 56),                # the stand-in trunk's images
    (2, 37, 51),                # odd H and W; Hc = 19 odd and Wc = 26 even: both parities of the pool's last window
    (1, 38, 50),
    SEAM_SHAPE,
    INTERIOR_SHAPE,
)
DTYPES = (torch.float32, torch.bfloat16)
DTYPE_IDS = ("f32", "bf16")


def out_hw(H, W):
    """(Hc, Wc, Hp, Wp) of an H x W image."""
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return Hc, Wc, (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1


def fragment_seam_pixels(k, tile=(0, 0)):
    """The two convolution pixels (cy, cx) of the map either side of fragment seam 16 k - 1 | 16 k of ``tile``
    (they may lie outside the map: row or column -1 of the first tile)."""
    out = []
    for p in (FRAG_PIX * k - 1, FRAG_PIX * k):
        out.append((2 * TILE * tile[0] - 1 + p // CONV_TILE, 2 * TILE * tile[1] - 1 + p % CONV_TILE))
    return out


def per_channel(t):
    return t.double().view(1, -1, 1, 1)


def conv7(x, w):
    return F.conv2d(x, w, None, stride=2, padding=3)


def pool3(a):
    return F.max_pool2d(a, 3, 2, 1)


def _finite(t):
    return torch.where(torch.isfinite(t), t, torch.zeros_like(t))


class StemCase:
    """Operands of one mvn_stem launch on the CPU: x (M, 3, H, W) f32, w (64, 3, 7, 7) bf16-exact f32, scale and
    shift (64,) f32.  ``x`` need not be bf16-exact: the contract rounds it."""

    def __init__(self, x, w, scale, shift):
        assert tuple(w.shape) == (COUT, CIN, KS, KS) and x.shape[1] == CIN and scale.shape == shift.shape == (COUT,)
        assert bool((w.bfloat16().float() == w).all())
        self.x, self.w, self.scale, self.shift = x, w, scale, shift

    def run(self, device, dtype=torch.float32, images=None, packed=None):
        from mvn_rocm import resnet
        if images is None:
            images = self.x.to(dtype).to(device)
        pk = resnet.pack_stem_weight(self.w.double()).to(device) if packed is None else packed
        return resnet.stem(images, pk, self.scale.to(device), self.shift.to(device))

    def pre_relu(self, f32=True):
        """fmaf(c, scale, shift) of the contract in float64, the convolution in f32 on the CPU or in float64."""
        xb = bf16r(self.x)
        acc = conv7(xb, self.w).double() if f32 else conv7(xb.double(), self.w.double())
        return acc * per_channel(self.scale) + per_channel(self.shift)

    def abs_terms(self):
        """S of the bound per convolution pixel: |scale| sum |x w| + |shift|, non-finite values left out."""
        return (conv7(_finite(bf16r(self.x)).double().abs(), self.w.double().abs()) * per_channel(self.scale).abs()
                + per_channel(self.shift).abs())

    def reference(self):
        """The bf16 (M, 64, Hp, Wp) result for operands on which no order of accumulation rounds: the sums of
        |x w| stay below 2^24 and the epilogue is exact in f32 (asserted)."""
        assert float(conv7(_finite(bf16r(self.x)).abs(), self.w.abs()).max()) <= K_REAL * 16 < 2.0 ** 24
        r = self.pre_relu()
        assert bool(((r.float().double() == r) | torch.isnan(r)).all()), "fma(c, scale, shift) is not exact in f32"
        assert not bool((torch.signbit(r) & (r == 0)).any()), "the pre-relu reference holds a -0"
        return pool3(relu64(r)).float().bfloat16()


def integer_case(shape, seed):
    """Integers in [-4, 4], scale +-2^k, shift in quarters: every sum is exact in f32 in any order."""
    M, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-4, 5, (M, CIN, H, W), generator=g).float()
    w = torch.randint(-4, 5, (COUT, CIN, KS, KS), generator=g).float()
    return StemCase(x, w, *exact_scale_shift(seed + 1, COUT))


def _seed(shape):
    return sum((7 * i + 3) * v for i, v in enumerate(shape))


@functools.lru_cache(maxsize=None)
def parity_case(shape):
    """The integer case of a shape and its reference, computed once and shared (read-only)."""
    case = integer_case(shape, _seed(shape))
    return case, case.reference()


def random_case(shape, seed, exact_inputs=True):
    """randn images (bf16-exact unless told otherwise), Xavier-sized weights times 3, scale in [0.75, 1.25] of
    both signs."""
    M, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, CIN, H, W, generator=g)
    w = bf16r(torch.randn(COUT, CIN, KS, KS, generator=g) * (2.0 / (K_REAL + COUT * KS * KS)) ** 0.5 * 3)
    scale = (0.75 + 0.5 * torch.rand(COUT, generator=g)) * torch.where(torch.arange(COUT) % 5 == 2, -1.0, 1.0)
    return StemCase(bf16r(x) if exact_inputs else x, w, scale, 0.2 * torch.randn(COUT, generator=g))


def check_bound(case, got, what):
    """got (M, 64, Hp, Wp) against the float64 restatement.  Per convolution pixel the bar is 2^-8 |a_ref| +
    gamma S: half a bf16 ulp of the one rounding plus the worst-case f32 bound of the 147 products and the fma,
    gamma = (147 + 1) 2^-24, S = |scale| sum |x w| + |shift|.  The maximum is 1-Lipschitz in the sup norm, so a
    pooled output's bar is the largest bar in its window.  The same convolution in f32 on the CPU must sit within
    0.05 of gamma S, so the bar is a bound for these inputs and no measurement.  Returns the worst fraction."""
    gamma, S = (K_REAL + 1) * 2.0 ** -24, case.abs_terms()
    r = case.pre_relu(f32=False)
    a = relu64(r)
    bar = pool3(2.0 ** -8 * a.abs() + gamma * S)
    ref = pool3(a)
    cpu_frac = float(((case.pre_relu(f32=True) - r).abs() / (gamma * S)).max())
    frac = float(((got.double() - ref).abs() / bar).max())
    print(f"{what}: worst |got - ref| / bar = {frac:.4f}; the f32 CPU convolution at {cpu_frac:.4f} of gamma S")
    assert cpu_frac <= 0.05, "the f32 CPU convolution is not far inside gamma S: the bar is no bound for these inputs"
    assert frac <= 1.0
    return frac


# ----------------------------------------------------------------------------- index weight, unpacker
def index_weight():
    """A bf16-exact (64, 3, 7, 7) weight that encodes its own index: the significand holds co (6 bits), the
    exponent the slot (ci 7 + ky) 7 + kx.  No two slots hold the same value."""
    co = torch.arange(COUT).view(-1, 1, 1, 1)
    slot = torch.arange(CIN * KS * KS).view(1, CIN, KS, KS)
    w = ((1.0 + co.double() / 64) * torch.exp2((slot - 74).double())).float().contiguous()
    assert bool((w.bfloat16().float() == w).all()) and w.unique().numel() == w.numel()
    return w


def slot_of(ci, ky, kx):
    """The documented K-slot of tap (ky, kx) of input channel ci."""
    return ROW_SLOTS * ky + CIN * kx + ci


def unpack_stem(packed):
    """((64, 3, 7, 7) weight, (64, 192) bool mask of the pad slots' non-zeros) from the documented layout
    (include/mvn_hip.h): [kp][m][lane][j] = A[16 m + (lane & 15)][32 kp + 8 (lane >> 4) + j],
    A[co][24 ky + 3 kx + ci] = w[co][ci][ky][kx]."""
    assert tuple(packed.shape) == (K_SLOTS // 32, COUT // 16, 64, 8) and packed.dtype == torch.bfloat16
    A = unpack_mfma_a(packed).permute(1, 0, 2).reshape(COUT, K_SLOTS)          # (kp, co, 32) -> (co, 192)
    w = torch.zeros(COUT, CIN, KS, KS, dtype=torch.float64)
    real = torch.zeros(K_SLOTS, dtype=torch.bool)
    for ci in range(CIN):
        for ky in range(KS):
            for kx in range(KS):
                w[:, ci, ky, kx] = A[:, slot_of(ci, ky, kx)]
                real[slot_of(ci, ky, kx)] = True
    assert int(real.sum()) == K_REAL
    return w, (A != 0) & ~real.view(1, -1)


def element(packed, kp, m, lane, j):
    """The documented element formula read literally: ((co, k), value)."""
    return (16 * m + (lane & 15), 32 * kp + 8 * (lane >> 4) + j), float(packed[kp, m, lane, j])


def cpu_stem(backbone, x):
    """The torch stem of ``backbone`` (conv1, bn1, relu, maxpool) on x (M, 3, H, W) as a ``StemCase``: the weight
    rounded to bf16, the BatchNorm folded in float64 and rounded once to f32."""
    bn = backbone.bn1
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
    b = backbone.conv1.bias.detach().double() if backbone.conv1.bias is not None else torch.zeros(COUT, dtype=torch.float64)
    t = (b - bn.running_mean.double()) * s + bn.bias.detach().double()
    return StemCase(x, bf16r(backbone.conv1.weight.detach()), s.float(), t.float())
