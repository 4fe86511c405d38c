"""Device time of the V2V's 128-channel levels on csrc/v2v_deep.hip (the 3x3x3 conv with 128 output
channels and the 128-channel upsample + skip add, any extent) against the stock torch.nn modules on
the GPU in eval mode, and of V2VEval.forward with deep="kernels" against half_res="kernels" alone.

    python tools/time_v2v_deep.py [--frames 8,32] [--repeats 5] [--calls 20] [--out FILE]
                                  [--no-model] [--no-pieces] [--no-stock]

The method of tools/time_v2v_interior.py: per measurement 10 warm-up calls, then HIP events around
`calls` back-to-back calls; the paths alternate in one process, `repeats` measurements each; the
table gives the median and the range (max - min) of the repeats.  The full resolution is 64^3, so
the levels run at 16^3, 8^3, 4^3 and 2^3.  The whole-model rows come first.  Piece rows: each conv
kind at 16^3; whole blocks at the four extents and the four upsamples + adds against the stock
modules in bf16 and f32, each in the faster of the contiguous and channels_last_3d formats (probed
with 3 + 5 calls, named in the row); the whole deep part (v2v_interior_deep_cl against
v2v_interior_deep with the glue around it).

Rooflines: bytes / 8 TB/s with the bytes of the row (a conv reads x and the skip and writes y; a
block also writes and reads the hidden volume; the packed weights once) and flop / 2.5 PF (dense
bf16)."""
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

from mvn_rocm import v2v, volumetric  # noqa: E402
from time_v2v_res3d import Res3DBlock, Upsample3DBlock, V2VModel, init, measure  # noqa: E402

V, J = 64, 17                            # full resolution, joints
HBM_BYTES_PER_S, BF16_FLOPS = 8e12, 2.5e15


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=lambda s: [int(x) for x in s.split(",")], default=[8, 32])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-model", action="store_true", help="skip the whole-model rows")
    ap.add_argument("--no-pieces", action="store_true", help="skip the per-kernel and per-block rows")
    ap.add_argument("--no-stock", action="store_true", help="time the kernels only, not the stock modules")
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

    emit(f"# 128-channel levels of the V2V (full resolution {V}^3: 16^3, 8^3, 4^3, 2^3); {args.repeats} repeats x "
         f"{args.calls} calls after 10 warm-up calls, paths alternating in one process; median us per call (device, "
         f"HIP events), spread = range of the repeats")
    emit(f"# {torch.cuda.get_device_name(0)}; roofline fractions: (bytes / 8 TB/s) / time and (flop / 2.5 PF) / time")
    with torch.no_grad():
        if not args.no_model:
            model = init(V2VModel(32, J))
            evs = {"deep": v2v.V2VEval.from_reference(model, device=dev, half_res="kernels", deep="kernels"),
                   "half_res": v2v.V2VEval.from_reference(model, device=dev, half_res="kernels")}
            for B in args.frames:
                emit(f"# whole model at {V}^3, B = {B}, J = {J}: V2VEval.forward (channels-last bf16 volume in), "
                     f"half_res=\"kernels\" with deep=\"kernels\" against half_res=\"kernels\" alone (f32 torch levels)")
                vol = torch.randn((B, V, V, V, 32), generator=torch.Generator().manual_seed(1)).to(torch.bfloat16).to(dev)
                coords = volumetric.build_coord_volumes(np.tile(np.array([[10.0, -20.0, 900.0]]), (B, 1)), 2500.0, V, device=dev)
                r = alternate({how: (lambda ev=ev: ev(vol, coords, 1.0)) for how, ev in evs.items()})
                for key, (us, spr) in r.items():
                    emit(f"{key:<10} {us:>12.1f} us  spread {spr:>9.1f}  ratio to half_res {us / r['half_res'][0]:>6.3f}")
                emit(f"difference half_res - deep {r['half_res'][0] - r['deep'][0]:>10.1f} us; sum of the two spreads "
                     f"{r['half_res'][1] + r['deep'][1]:>8.1f} us")
                # the deep part alone, both ways, on inputs of the right shapes
                e1 = torch.randn((B, V // 2, V // 2, V // 2, 64), generator=torch.Generator().manual_seed(2)).to(torch.bfloat16).to(dev)
                s2 = torch.randn_like(e1)
                ed, deep = evs["half_res"].interior, evs["deep"].deep

                def torch_deep():
                    d = v2v.v2v_interior_deep(ed, e1.permute(0, 4, 1, 2, 3).float()) + s2.permute(0, 4, 1, 2, 3)
                    return d.permute(0, 2, 3, 4, 1).to(torch.bfloat16).contiguous()
                r = alternate({"deep levels, kernels (32 launches)": lambda: v2v.v2v_interior_deep_cl(deep, e1, s2),
                               "deep levels, torch f32 + glue": torch_deep,
                               "whole trunk, deep": lambda: evs["deep"].trunk(vol),
                               "whole trunk, half_res": lambda: evs["half_res"].trunk(vol)})
                for key, (us, spr) in r.items():
                    emit(f"{key:<38} {us:>12.1f} us  spread {spr:>9.1f}")
                del vol, coords, e1, s2
                torch.cuda.empty_cache()

        if not args.no_pieces:
            blocks = {64: init(Res3DBlock(64, 128)), 128: init(Res3DBlock(128, 128))}
            ups = {128: init(Upsample3DBlock(128, 128)), 64: init(Upsample3DBlock(128, 64))}
            params = {c: v2v.fold_res3d_block_deep(b, device=dev) for c, b in blocks.items()}
            pus = {c: v2v.fold_upsample_block_deep(u, device=dev) for c, u in ups.items()}
            hdr = (f"{'row':<30} {'B':>3} {'us':>10} {'spread':>8} {'MB':>8} {'of 8 TB/s':>9} {'GFLOP':>8} {'of 2.5 PF':>9} "
                   f"{'stock bf16 us':>14} {'spread':>8} {'ratio':>6} {'stock f32 us':>13} {'spread':>8} {'ratio':>6}  stock formats")
            for B in args.frames:
                emit(hdr)
                g = torch.Generator().manual_seed(B)

                def rnd(D, c):
                    return torch.randn((B, D, D, D, c), generator=g).to(torch.bfloat16).to(dev)

                def stock_fn(make, xin, dt, extra=None):
                    """make() -> a stock module; run in dtype dt on the NCDHW view of xin, in the faster format."""
                    best = None
                    for name, fmt in (("contiguous", torch.contiguous_format), ("channels_last_3d", torch.channels_last_3d)):
                        m = make().to(dev).to(dt).to(memory_format=fmt)
                        xi = xin.permute(0, 4, 1, 2, 3).to(dt).contiguous(memory_format=fmt)
                        ei = extra.permute(0, 4, 1, 2, 3).to(dt).contiguous(memory_format=fmt) if extra is not None else None

                        def run(m=m, xi=xi, ei=ei):
                            y = m(xi)
                            return y + ei if ei is not None else y
                        t = measure(run, 5, warm=3)
                        if best is None or t < best[0]:
                            best = (t, name, run)
                    return best[2], best[1]

                p64, p128 = params[64], params[128]
                wbytes = lambda cin: 27 * cin * 128 * 2                                                # noqa: E731
                rows = []          # (name, fn, bytes, flop, stock: (make, input, extra) or None)
                D = 16
                nvox = B * D ** 3
                x64, x128 = rnd(D, 64), rnd(D, 128)
                cf = lambda cin, n: 2 * 27 * cin * 128 * n                                             # noqa: E731
                pw = lambda n: 2 * 64 * 128 * n                                                        # noqa: E731
                rows.append(("conv3_deep 64 none 16^3", lambda: v2v.v2v_conv3_deep(x64, p64.packed1, p64.scale1, p64.shift1),
                             nvox * (128 + 256) + wbytes(64), cf(64, nvox), None))
                rows.append(("conv3_deep 128 none 16^3", lambda: v2v.v2v_conv3_deep(x128, p128.packed1, p128.scale1, p128.shift1),
                             nvox * 512 + wbytes(128), cf(128, nvox), None))
                rows.append(("conv3_deep 128 identity 16^3",
                             lambda: v2v.v2v_conv3_deep(x128, p128.packed2, p128.scale2, p128.shift2, x128),
                             nvox * 768 + wbytes(128), cf(128, nvox), None))
                rows.append(("conv3_deep 128 pointwise 16^3",
                             lambda: v2v.v2v_conv3_deep(x128, p64.packed2, p64.scale2, p64.shift2, x64, p64.skip_packed,
                                                        p64.skip_scale, p64.skip_shift),
                             nvox * (512 + 128) + wbytes(128), cf(128, nvox) + pw(nvox), None))
                rows.append(("block 64->128 pointwise 16^3", lambda: v2v.res3d_block_deep(x64, p64),
                             nvox * (128 + 256 + 256 + 128 + 256) + wbytes(64) + wbytes(128),
                             cf(64, nvox) + cf(128, nvox) + pw(nvox), (lambda: copy.deepcopy(blocks[64]), x64, None)))
                for D in (16, 8, 4, 2):
                    n = B * D ** 3
                    xi = x128 if D == 16 else rnd(D, 128)
                    rows.append((f"block 128->128 identity {D}^3", lambda xi=xi: v2v.res3d_block_deep(xi, p128),
                                 n * 256 * 5 + 2 * wbytes(128), 2 * cf(128, n), (lambda: copy.deepcopy(blocks[128]), xi, None)))
                for D, cout in ((1, 128), (2, 128), (4, 128), (8, 64)):
                    n = B * D ** 3
                    xi, sk = rnd(D, 128), rnd(2 * D, cout)
                    rows.append((f"upsample {D}^3->{2 * D}^3 x {cout} + skip",
                                 lambda xi=xi, sk=sk, cout=cout: v2v.upsample2_add_deep(xi, pus[cout], sk),
                                 n * 256 + 8 * n * cout * 4 + 128 * cout * 16, 2 * 128 * 8 * cout * n,
                                 (lambda cout=cout: copy.deepcopy(ups[cout]), xi, sk)))
                for name, fn, nbytes, flop, stock in rows:
                    fns, fmts = {"ours": fn}, []
                    if stock is not None and not args.no_stock:
                        for key, dt in (("bf16", torch.bfloat16), ("f32", torch.float32)):
                            fns[key], fmt = stock_fn(stock[0], stock[1], dt, stock[2])
                            fmts.append(f"{key}: {fmt}")
                    r = alternate(fns)
                    us, spr = r["ours"]
                    line = (f"{name:<30} {B:>3} {us:>10.1f} {spr:>8.1f} {nbytes / 1e6:>8.2f} {nbytes / HBM_BYTES_PER_S * 1e6 / us:>9.3f} "
                            f"{flop / 1e9:>8.2f} {flop / BF16_FLOPS * 1e6 / us:>9.3f}")
                    for key in ("bf16", "f32"):
                        line += (f" {r[key][0]:>14.1f} {r[key][1]:>8.1f} {us / r[key][0]:>6.3f}" if key in r
                                 else f" {'-':>14} {'-':>8} {'-':>6}")
                    emit(line + "  " + ", ".join(fmts))
                    del fns
                    torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
