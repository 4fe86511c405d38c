"""Device time of the full-resolution Res3DBlocks on csrc/v2v_res3d.hip against the stock torch.nn
modules of the same block on the GPU in eval mode, and of V2VEval.forward against the stock
V2VModel forward followed by mvn_rocm.op.integrate_tensor_3d_with_coordinates.

    python tools/time_v2v_res3d.py [--frames 8,32] [--repeats 5] [--calls 20] [--out FILE] [--no-model]

64^3.  Per measurement: 10 warm-up calls, then HIP events around `calls` back-to-back calls; the
paths alternate in one process, `repeats` measurements each; the table gives the median and the
range (max - min) of the repeats.  Rows: one mvn_v2v_conv3 launch per mode, the one-call block for
both block shapes (16 -> 32 with the pointwise skip, 32 -> 32 with the identity skip), and the
five full-resolution blocks of the V2V in sequence (front_layers[1..3], skip_res1, back_layers[0]:
one 16 -> 32 and four 32 -> 32).  The stock baseline is a torch.nn Res3DBlock in bf16 and in f32,
in the faster of the contiguous and channels_last_3d memory formats (probed with 3 + 5 calls,
named in the row).

Rooflines: bytes / 8 TB/s with the bytes of the row stated (a conv reads x and the skip and
writes y; a block also writes and reads the hidden volume), and flop / 2.5 PF (dense bf16), flop =
2 * 27 * cin * 32 per voxel and conv (+ 2 * 16 * 32 for the pointwise skip)."""
import argparse
import copy
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "learnable-triangulation-pytorch_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch import nn  # noqa: E402

from mvn_rocm import op, v2v, volumetric  # noqa: E402

V, J, C = 64, 17, 32
HBM_BYTES_PER_S, BF16_FLOPS = 8e12, 2.5e15


class Basic3DBlock(nn.Module):
    def __init__(self, cin, cout, k):
        super().__init__()
        self.block = nn.Sequential(nn.Conv3d(cin, cout, k, 1, (k - 1) // 2), nn.BatchNorm3d(cout), nn.ReLU(True))

    def forward(self, x):
        return self.block(x)


class Res3DBlock(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.res_branch = nn.Sequential(nn.Conv3d(cin, cout, 3, 1, 1), nn.BatchNorm3d(cout), nn.ReLU(True),
                                        nn.Conv3d(cout, cout, 3, 1, 1), nn.BatchNorm3d(cout))
        self.skip_con = nn.Sequential() if cin == cout else nn.Sequential(nn.Conv3d(cin, cout, 1), nn.BatchNorm3d(cout))

    def forward(self, x):
        return F.relu(self.res_branch(x) + self.skip_con(x), True)


class Pool3DBlock(nn.Module):
    def forward(self, x):
        return F.max_pool3d(x, kernel_size=2, stride=2)


class Upsample3DBlock(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.block = nn.Sequential(nn.ConvTranspose3d(cin, cout, 2, 2), nn.BatchNorm3d(cout), nn.ReLU(True))

    def forward(self, x):
        return self.block(x)


class EncoderDecorder(nn.Module):
    def __init__(self):
        super().__init__()
        ch = [32, 64, 128, 128, 128, 128]
        for i in range(1, 6):
            setattr(self, f"encoder_pool{i}", Pool3DBlock())
            setattr(self, f"encoder_res{i}", Res3DBlock(ch[i - 1], ch[i]))
            setattr(self, f"decoder_res{i}", Res3DBlock(ch[i], ch[i]))
            setattr(self, f"decoder_upsample{i}", Upsample3DBlock(ch[i], ch[i - 1]))
            setattr(self, f"skip_res{i}", Res3DBlock(ch[i - 1], ch[i - 1]))
        self.mid_res = Res3DBlock(128, 128)

    def forward(self, x):
        skips = []
        for i in range(1, 6):
            skips.append(getattr(self, f"skip_res{i}")(x))
            x = getattr(self, f"encoder_res{i}")(getattr(self, f"encoder_pool{i}")(x))
        x = self.mid_res(x)
        for i in range(5, 0, -1):
            x = getattr(self, f"decoder_upsample{i}")(getattr(self, f"decoder_res{i}")(x)) + skips[i - 1]
        return x


class V2VModel(nn.Module):
    def __init__(self, cin, n_joints):
        super().__init__()
        self.front_layers = nn.Sequential(Basic3DBlock(cin, 16, 7), Res3DBlock(16, 32), Res3DBlock(32, 32),
                                          Res3DBlock(32, 32))
        self.encoder_decoder = EncoderDecorder()
        self.back_layers = nn.Sequential(Res3DBlock(32, 32), Basic3DBlock(32, 32, 1), Basic3DBlock(32, 32, 1))
        self.output_layer = nn.Conv3d(32, n_joints, 1)

    def forward(self, x):
        return self.output_layer(self.back_layers(self.encoder_decoder(self.front_layers(x))))


def init(module):
    torch.manual_seed(0)
    for c in module.modules():
        if isinstance(c, (nn.Conv3d, nn.ConvTranspose3d)):
            nn.init.xavier_normal_(c.weight)
        elif isinstance(c, nn.BatchNorm3d):
            c.running_mean.normal_(0, 0.2)
            c.running_var.uniform_(0.75, 1.25)
    return module.eval()


def measure(fn, calls, warm=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls * 1e3                      # us per call


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=lambda s: [int(x) for x in s.split(",")], default=[8, 32])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-model", action="store_true", help="skip the whole-model rows")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = None
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        out = open(args.out, "w")

    def emit(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    def alternate(fns):
        res = {k: [] for k in fns}
        for _ in range(args.repeats):
            for k, fn in fns.items():
                res[k].append(measure(fn, args.calls))
        return {k: (statistics.median(v), max(v) - min(v)) for k, v in res.items()}

    emit(f"# full-resolution Res3DBlocks at {V}^3; {args.repeats} repeats x {args.calls} calls after 10 warm-up calls, "
         f"paths alternating in one process; median us per call (device, HIP events), spread = range of the repeats")
    emit(f"# {torch.cuda.get_device_name(0)}; roofline fractions: (bytes / 8 TB/s) / time and (flop / 2.5 PF) / time")
    blocks = {16: init(Res3DBlock(16, C)), 32: init(Res3DBlock(C, C))}
    params = {c: v2v.fold_res3d_block(b, device=dev) for c, b in blocks.items()}
    hdr = (f"{'row':<28} {'B':>3} {'us':>10} {'spread':>8} {'MB':>8} {'of 8 TB/s':>9} {'GFLOP':>8} {'of 2.5 PF':>9} "
           f"{'stock bf16 us':>14} {'spread':>8} {'ratio':>6} {'stock f32 us':>13} {'spread':>8} {'ratio':>6}  stock formats")
    with torch.no_grad():
        for B in args.frames:
            emit(hdr)
            g = torch.Generator().manual_seed(B)
            x = {c: torch.randn((B, V, V, V, c), generator=g).to(torch.bfloat16).to(dev) for c in (16, 32)}
            nvox = B * V ** 3
            p16, p32 = params[16], params[32]

            def stock_fn(seq, cin, dt):
                """The stock modules `seq` in dtype dt on an NCDHW input, in the faster memory format."""
                best = None
                for name, fmt in (("contiguous", torch.contiguous_format), ("channels_last_3d", torch.channels_last_3d)):
                    ms = [copy.deepcopy(blocks[c]).to(dev).to(dt).to(memory_format=fmt) for c in seq]
                    xi = x[cin].permute(0, 4, 1, 2, 3).to(dt).contiguous(memory_format=fmt)

                    def run(ms=ms, xi=xi):
                        h = xi
                        for m in ms:
                            h = m(h)
                        return h
                    t = measure(run, 5, warm=3)
                    if best is None or t < best[0]:
                        best = (t, name, run)
                return best[2], best[1]

            rows = []          # (name, fn, bytes, flop, stock sequence or None, stock cin)
            conv_flop = lambda cin: 2 * 27 * cin * C * nvox                                   # noqa: E731
            rows.append(("conv3 32 none", lambda: v2v.v2v_conv3(x[32], p32.packed1, p32.scale1, p32.shift1),
                         nvox * (64 + 64), conv_flop(32), None, 0))
            rows.append(("conv3 16 none", lambda: v2v.v2v_conv3(x[16], p16.packed1, p16.scale1, p16.shift1),
                         nvox * (32 + 64), conv_flop(16), None, 0))
            rows.append(("conv3 32 identity", lambda: v2v.v2v_conv3(x[32], p32.packed2, p32.scale2, p32.shift2, x[32]),
                         nvox * (64 + 64 + 64), conv_flop(32), None, 0))
            rows.append(("conv3 32 pointwise", lambda: v2v.v2v_conv3(x[32], p16.packed2, p16.scale2, p16.shift2, x[16],
                                                                     p16.skip_packed, p16.skip_scale, p16.skip_shift),
                         nvox * (64 + 32 + 64), conv_flop(32) + 2 * 16 * C * nvox, None, 0))
            rows.append(("block 16->32 pointwise", lambda: v2v.res3d_block(x[16], p16),
                         nvox * (32 + 64 + 64 + 32 + 64), conv_flop(16) + conv_flop(32) + 2 * 16 * C * nvox, (16,), 16))
            rows.append(("block 32->32 identity", lambda: v2v.res3d_block(x[32], p32),
                         nvox * 64 * 5, 2 * conv_flop(32), (32,), 32))

            def five():
                h = v2v.res3d_block(x[16], p16)
                for _ in range(4):
                    h = v2v.res3d_block(h, p32)
                return h
            rows.append(("five blocks in sequence", five, nvox * (256 + 4 * 320),
                         conv_flop(16) + 9 * conv_flop(32) + 2 * 16 * C * nvox, (16, 32, 32, 32, 32), 16))
            for name, fn, nbytes, flop, seq, cin in rows:
                fns, fmts = {"ours": fn}, []
                if seq is not None:
                    for key, dt in (("bf16", torch.bfloat16), ("f32", torch.float32)):
                        fns[key], fmt = stock_fn(seq, cin, dt)
                        fmts.append(f"{key}: {fmt}")
                r = alternate(fns)
                us, spr = r["ours"]
                line = (f"{name:<28} {B:>3} {us:>10.1f} {spr:>8.1f} {nbytes / 1e6:>8.1f} {nbytes / HBM_BYTES_PER_S * 1e6 / us:>9.3f} "
                        f"{flop / 1e9:>8.1f} {flop / BF16_FLOPS * 1e6 / us:>9.3f}")
                for key in ("bf16", "f32"):
                    line += (f" {r[key][0]:>14.1f} {r[key][1]:>8.1f} {us / r[key][0]:>6.3f}" if key in r
                             else f" {'-':>14} {'-':>8} {'-':>6}")
                emit(line + "  " + ", ".join(fmts))
                del fns
                torch.cuda.empty_cache()
            del x
            torch.cuda.empty_cache()

        if not args.no_model:
            B = 8
            emit(f"# whole model at {V}^3, B = {B}, J = {J}: V2VEval.forward (channels-last bf16 volume in, f32 interior) "
                 f"against the stock V2VModel forward + op.integrate_tensor_3d_with_coordinates (NCDHW volume in)")
            model = init(V2VModel(C, J))
            ev = v2v.V2VEval.from_reference(model, device=dev)
            vol = torch.randn((B, V, V, V, C), generator=torch.Generator().manual_seed(1)).to(torch.bfloat16).to(dev)
            coords = volumetric.build_coord_volumes(np.tile(np.array([[10.0, -20.0, 900.0]]), (B, 1)), 2500.0, V, device=dev)
            fns = {"V2VEval": lambda: ev(vol, coords, 1.0)}
            for key, dt in (("stock bf16", torch.bfloat16), ("stock f32", torch.float32)):
                md = copy.deepcopy(model).to(dev).to(dt)
                xi = vol.permute(0, 4, 1, 2, 3).to(dt).contiguous()
                fns[key] = lambda md=md, xi=xi: op.integrate_tensor_3d_with_coordinates(md(xi), coords, True, multiplier=1.0)
            r = alternate(fns)
            for key, (us, spr) in r.items():
                emit(f"{key:<12} {us:>12.1f} us  spread {spr:>9.1f}  ratio to V2VEval {us / r['V2VEval'][0]:>6.3f}")
    if out:
        out.close()


if __name__ == "__main__":
    main()
