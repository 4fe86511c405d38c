"""Device time of the V2V's first pooled level on csrc/v2v_interior.hip (the channels-last max
pool, the 64-channel 3x3x3 conv, the fused upsample + skip add) against the stock torch.nn modules
on the GPU in eval mode, and of V2VEval.forward with half_res="kernels" against half_res="torch".

    python tools/time_v2v_interior.py [--frames 8,32] [--repeats 5] [--calls 20] [--out FILE] [--no-model]

The method of tools/time_v2v_res3d.py: per measurement 10 warm-up calls, then HIP events around
`calls` back-to-back calls; the paths alternate in one process, `repeats` measurements each; the
table gives the median and the range (max - min) of the repeats.  The full resolution is 64^3, so
the level runs at 32^3.  Rows: each kernel alone; each wide block (32 -> 64 with the pointwise skip,
64 -> 64 with the identity skip), the pool and the upsample + add against the stock modules in bf16
and f32, each in the faster of the contiguous and channels_last_3d formats (probed with 3 + 5
calls, named in the row); V2VEval.forward both ways; and the pieces of the torch path (the level's
modules, the deeper levels, the full-size glue) for the split of the difference.

Rooflines: bytes / 8 TB/s with the bytes of the row (a conv reads x and the skip and writes y; a
block also writes and reads the hidden volume) and flop / 2.5 PF (dense bf16)."""
import argparse
import copy
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "learnable-triangulation-pytorch_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from mvn_rocm import v2v, volumetric  # noqa: E402
from time_v2v_res3d import Res3DBlock, Upsample3DBlock, V2VModel, init, measure  # noqa: E402

V, H, J = 64, 32, 17                     # full resolution, the level's resolution, joints
HBM_BYTES_PER_S, BF16_FLOPS = 8e12, 2.5e15


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

    emit(f"# first pooled level of the V2V at {H}^3 (full resolution {V}^3); {args.repeats} repeats x {args.calls} calls "
         f"after 10 warm-up calls, paths alternating in one process; median us per call (device, HIP events), "
         f"spread = range of the repeats")
    emit(f"# {torch.cuda.get_device_name(0)}; roofline fractions: (bytes / 8 TB/s) / time and (flop / 2.5 PF) / time")
    blocks = {32: init(Res3DBlock(32, 64)), 64: init(Res3DBlock(64, 64))}
    up = init(Upsample3DBlock(64, 32))
    params = {c: v2v.fold_res3d_block_wide(b, device=dev) for c, b in blocks.items()}
    pu = v2v.fold_upsample_block(up, device=dev)
    hdr = (f"{'row':<28} {'B':>3} {'us':>10} {'spread':>8} {'MB':>8} {'of 8 TB/s':>9} {'GFLOP':>8} {'of 2.5 PF':>9} "
           f"{'stock bf16 us':>14} {'spread':>8} {'ratio':>6} {'stock f32 us':>13} {'spread':>8} {'ratio':>6}  stock formats")
    with torch.no_grad():
        for B in args.frames:
            emit(hdr)
            g = torch.Generator().manual_seed(B)
            x = {c: torch.randn((B, H, H, H, c), generator=g).to(torch.bfloat16).to(dev) for c in (32, 64)}
            full = torch.randn((B, V, V, V, 32), generator=g).to(torch.bfloat16).to(dev)
            nvox = B * H ** 3
            p32, p64 = params[32], params[64]

            def stock_fn(make, xin, dt, extra=None):
                """make() -> a stock module; run in dtype dt on the NCDHW view of xin, in the faster format."""
                best = None
                for name, fmt in (("contiguous", torch.contiguous_format), ("channels_last_3d", torch.channels_last_3d)):
                    m = make().to(dev).to(dt).to(memory_format=fmt) if make is not None else None
                    xi = xin.permute(0, 4, 1, 2, 3).to(dt).contiguous(memory_format=fmt)
                    ei = extra.permute(0, 4, 1, 2, 3).to(dt).contiguous(memory_format=fmt) if extra is not None else None

                    def run(m=m, xi=xi, ei=ei):
                        y = m(xi) if m is not None else F.max_pool3d(xi, 2, 2)
                        return y + ei if ei is not None else y
                    t = measure(run, 5, warm=3)
                    if best is None or t < best[0]:
                        best = (t, name, run)
                return best[2], best[1]

            conv_flop = lambda cin: 2 * 27 * cin * 64 * nvox                                  # noqa: E731
            pw_flop = 2 * 32 * 64 * nvox
            rows = []          # (name, fn, bytes, flop, stock: (make, input, extra) or None)
            rows.append(("maxpool2 64^3 x 32", lambda: v2v.max_pool2_cl(full), B * V ** 3 * 64 + nvox * 64, 0,
                         (None, full, None)))
            rows.append(("conv3_wide 32 none", lambda: v2v.v2v_conv3_wide(x[32], p32.packed1, p32.scale1, p32.shift1),
                         nvox * (64 + 128), conv_flop(32), None))
            rows.append(("conv3_wide 64 none", lambda: v2v.v2v_conv3_wide(x[64], p64.packed1, p64.scale1, p64.shift1),
                         nvox * (128 + 128), conv_flop(64), None))
            rows.append(("conv3_wide 64 identity", lambda: v2v.v2v_conv3_wide(x[64], p64.packed2, p64.scale2, p64.shift2, x[64]),
                         nvox * (128 * 3), conv_flop(64), None))
            rows.append(("conv3_wide 64 pointwise", lambda: v2v.v2v_conv3_wide(x[64], p32.packed2, p32.scale2, p32.shift2, x[32],
                                                                               p32.skip_packed, p32.skip_scale, p32.skip_shift),
                         nvox * (128 + 64 + 128), conv_flop(64) + pw_flop, None))
            rows.append(("block 32->64 pointwise", lambda: v2v.res3d_block_wide(x[32], p32),
                         nvox * (64 + 128 + 128 + 64 + 128), conv_flop(32) + conv_flop(64) + pw_flop,
                         (lambda: copy.deepcopy(blocks[32]), x[32], None)))
            rows.append(("block 64->64 identity", lambda: v2v.res3d_block_wide(x[64], p64),
                         nvox * 128 * 5, 2 * conv_flop(64), (lambda: copy.deepcopy(blocks[64]), x[64], None)))
            rows.append(("upsample2 + skip", lambda: v2v.upsample2_add(x[64], pu, full),
                         nvox * 128 + B * V ** 3 * 128, 2 * 64 * 256 * nvox, (lambda: copy.deepcopy(up), x[64], full)))
            for name, fn, nbytes, flop, stock in rows:
                fns, fmts = {"ours": fn}, []
                if stock is not None:
                    for key, dt in (("bf16", torch.bfloat16), ("f32", torch.float32)):
                        fns[key], fmt = stock_fn(stock[0], stock[1], dt, stock[2])
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
            del x, full
            torch.cuda.empty_cache()

        if not args.no_model:
            model = init(V2VModel(32, J))
            evs = {how: v2v.V2VEval.from_reference(model, device=dev, half_res=how) for how in ("kernels", "torch")}
            for B in args.frames:
                emit(f"# whole model at {V}^3, B = {B}, J = {J}: V2VEval.forward (channels-last bf16 volume in, f32 interior), "
                     f"half_res=\"kernels\" against half_res=\"torch\"")
                vol = torch.randn((B, V, V, V, 32), generator=torch.Generator().manual_seed(1)).to(torch.bfloat16).to(dev)
                coords = volumetric.build_coord_volumes(np.tile(np.array([[10.0, -20.0, 900.0]]), (B, 1)), 2500.0, V, device=dev)
                r = alternate({how: (lambda ev=ev: ev(vol, coords, 1.0)) for how, ev in evs.items()})
                for key, (us, spr) in r.items():
                    emit(f"half_res={key:<8} {us:>12.1f} us  spread {spr:>9.1f}  ratio to torch {us / r['torch'][0]:>6.3f}")
                emit(f"difference torch - kernels {r['torch'][0] - r['kernels'][0]:>10.1f} us; sum of the two spreads "
                     f"{r['torch'][1] + r['kernels'][1]:>8.1f} us")
                # where the torch path's time goes: its pieces alone, on inputs of the right shapes
                ed = evs["torch"].interior
                h = torch.randn((B, V, V, V, 32), generator=torch.Generator().manual_seed(2)).to(torch.bfloat16).to(dev)
                s1 = torch.randn_like(h)
                hf = h.permute(0, 4, 1, 2, 3).float()
                e1 = ed.encoder_res1(ed.encoder_pool1(hf))
                d = v2v.v2v_interior_deep(ed, e1)
                u = ed.decoder_upsample1(ed.decoder_res1(d))
                pieces = {
                    "cast 64^3 x 32 to f32 NCDHW": lambda: h.permute(0, 4, 1, 2, 3).float(),
                    "pool1 + encoder_res1": lambda: ed.encoder_res1(ed.encoder_pool1(hf)),
                    "skip_res2": lambda: ed.skip_res2(e1),
                    "deeper levels (16^3 and below)": lambda: v2v.v2v_interior_deep(ed, e1),
                    "decoder_res1 + upsample1": lambda: ed.decoder_upsample1(ed.decoder_res1(d)),
                    "+ skip_x1, cast to bf16 NDHWC": lambda: (u + s1.permute(0, 4, 1, 2, 3)).permute(0, 2, 3, 4, 1).to(torch.bfloat16).contiguous(),
                    "whole trunk, torch": lambda: evs["torch"].trunk(vol),
                    "whole trunk, kernels": lambda: evs["kernels"].trunk(vol),
                }
                r = alternate(pieces)
                emit(f"# pieces of the half_res=\"torch\" path at B = {B} (f32, the model's modules), us")
                for key, (us, spr) in r.items():
                    emit(f"{key:<34} {us:>12.1f} us  spread {spr:>9.1f}")
                del vol, coords, h, s1, hf, e1, d, u, pieces
                torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
