"""Device time of the V2V head with the soft-argmax behind it: the one-call path
(mvn_rocm.v2v.v2v_head_softargmax) against the same tail as stock torch modules on the GPU in eval
mode (Basic3DBlock(32, 32, 1) twice, Conv3d(32, J, 1)) followed by
mvn_rocm.op.integrate_tensor_3d_with_coordinates.

    python tools/time_v2v_head.py [--frames 8,32] [--dtypes f32,bf16] [--repeats 5] [--calls 20] [--out FILE]

64^3, J = 17, softmax, volumes returned, multiplier 1.  Per measurement: 10 warm-up calls, then HIP
events around `calls` back-to-back calls; the paths alternate in one process, `repeats`
measurements each; the table gives the median and the range (max - min) of the repeats.  The stock
path runs in the same dtype as the fused one reads (module weights cast to it).  Also timed: the
head kernel alone (f32 logits) and the soft-argmax alone on its logits.

Roofline: the algorithm's HBM bytes per frame are x once, the logits written once and read twice
(the soft-argmax's two passes) and the volume written once, against 8 TB/s."""
import argparse
import copy
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "learnable-triangulation-pytorch_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch import nn  # noqa: E402

from mvn_rocm import op, v2v, volumetric  # noqa: E402

V, J, C = 64, 17, 32
HBM_BYTES_PER_S = 8e12


class Basic3DBlock(nn.Module):
    def __init__(self, cin, cout, k):
        super().__init__()
        self.block = nn.Sequential(nn.Conv3d(cin, cout, k, 1, (k - 1) // 2), nn.BatchNorm3d(cout), nn.ReLU(True))

    def forward(self, x):
        return self.block(x)


def make_modules():
    torch.manual_seed(0)
    mods = [Basic3DBlock(C, C, 1), Basic3DBlock(C, C, 1), nn.Conv3d(C, J, 1)]
    for m in mods:
        for c in m.modules():
            if isinstance(c, nn.Conv3d):
                nn.init.xavier_normal_(c.weight)
            elif isinstance(c, nn.BatchNorm3d):
                c.running_mean.normal_(0, 0.2)
                c.running_var.uniform_(0.75, 1.25)
        m.eval()
    return mods


def measure(fn, calls):
    for _ in range(10):
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
    ap.add_argument("--dtypes", type=lambda s: s.split(","), default=["f32", "bf16"])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# V2V head + soft-argmax at {V}^3, J = {J}, softmax, volumes returned; {args.repeats} repeats x {args.calls} "
         f"calls, alternating; median us per call (device, HIP events), spread = range of the repeats")
    emit(f"# {torch.cuda.get_device_name(0)}")
    emit(f"{'dtype':>5} {'B':>3} {'stock us':>10} {'spread':>7} {'fused us':>9} {'spread':>7} {'fused/stock':>11} "
         f"{'head us':>8} {'softargmax us':>13} {'roofline us':>11} {'fused/roofline':>14}  joints max|diff| mm")
    mods = make_modules()
    for name in args.dtypes:
        dt = {"f32": torch.float32, "bf16": torch.bfloat16}[name]
        es = 4 if dt == torch.float32 else 2
        stock = [copy.deepcopy(m).to(dev).to(dt) for m in mods]
        params = v2v.fold_v2v_head(*mods, device=dev)
        for B in args.frames:
            x = torch.randn((B, C, V, V, V), generator=torch.Generator().manual_seed(B)).to(dev).to(dt)
            base = np.tile(np.array([[10.0, -20.0, 900.0]]), (B, 1))
            coords = volumetric.build_coord_volumes(base, 2500.0, V, device=dev)
            with torch.no_grad():
                def run_stock():
                    return op.integrate_tensor_3d_with_coordinates(stock[2](stock[1](stock[0](x))), coords, True,
                                                                   multiplier=1.0)

                def run_fused():
                    return v2v.v2v_head_softargmax(x, *params, coords, multiplier=1.0, out_dtype=dt)

                def run_head():
                    return v2v.v2v_head(x, *params)
                logits = run_head()

                def run_sa():
                    return op.integrate_tensor_3d_with_coordinates(logits, coords, True, multiplier=1.0)
                diff = float((run_stock()[0].float() - run_fused()[0]).abs().max())
                fns = {"stock": run_stock, "fused": run_fused, "head": run_head, "sa": run_sa}
                res = {k: [] for k in fns}
                for _ in range(args.repeats):
                    for k, fn in fns.items():
                        res[k].append(measure(fn, args.calls))
            med = {k: statistics.median(v) for k, v in res.items()}
            spr = {k: max(v) - min(v) for k, v in res.items()}
            # bytes: x once; logits written once, read twice; the volume written once (logits f32
            # unless a bf16 volume is asked for, then bf16)
            le = 2 if dt == torch.bfloat16 else 4
            nbytes = B * V ** 3 * (C * es + J * le * 3 + J * es)
            roof = nbytes / HBM_BYTES_PER_S * 1e6
            emit(f"{name:>5} {B:>3} {med['stock']:>10.1f} {spr['stock']:>7.1f} {med['fused']:>9.1f} {spr['fused']:>7.1f} "
                 f"{med['fused'] / med['stock']:>11.3f} {med['head']:>8.1f} {med['sa']:>13.1f} {roof:>11.1f} "
                 f"{med['fused'] / roof:>14.2f}  {diff:.4f}")
            del x, coords, logits
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
