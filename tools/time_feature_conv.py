"""Device time of the feature convolution (csrc/feature_conv.hip, Conv2d(256, 32, 1) on the f32
MFMA) against the path it replaces, F.conv2d on the GPU, and of model.VolumetricEval.forward against
the four calls it replaces.

    python tools/time_feature_conv.py [--frames 8,32] [--repeats 5] [--calls 20] [--out FILE] [--no-model]

The method of tools/time_v2v_deep.py: per measurement 10 warm-up calls, then HIP events around
`calls` back-to-back calls; the paths alternate in one process, `repeats` measurements each; the
table gives the median and the range (max - min) of the repeats.

Kernel rows: B frames x 4 views of 256 x 96^2 maps, f32 -> f32, f32 -> bf16 and bf16 -> bf16.  The
torch path is F.conv2d in the input's dtype, followed by .to(bfloat16) where an f32 conv feeds a
bf16 result, with the maps in the default and in the channels_last memory format (prepared outside
the timed region).  Per kernel row: the fraction of 8 TB/s on the algorithmic bytes (x once, y
once, the weight once) and the fraction of the MFMA floor (one v_mfma_f32_32x32x2_f32 of 64 cycles
per 32 pixels and 2 input channels, on 1,024 SIMDs at 2.4 GHz).

Whole-module rows: VolumetricEval.forward (feature_dtype bf16 and f32) at 64^3, J = 17, softmax
aggregation, cuboids, against F.conv2d in f32, .to(bfloat16), v2v.unproject_channels_last and
V2VEval.forward."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "learnable-triangulation-pytorch_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch import nn  # noqa: E402

from mvn_rocm import model, synth, v2v  # noqa: E402
from time_v2v_res3d import V2VModel, init, measure  # noqa: E402

N, CIN, HM, V, J = 4, 256, 96, 64, 17
HBM_BYTES_PER_S, SIMDS, CLOCK_HZ, MFMA_CYCLES = 8e12, 1024, 2.4e9, 64


class Net(nn.Module):
    """What VolumetricEval.from_reference reads of VolumetricTriangulationNet."""

    def __init__(self):
        super().__init__()
        self.process_features = nn.Sequential(nn.Conv2d(CIN, 32, 1))
        self.volume_net = init(V2VModel(32, J))
        self.volume_aggregation_method, self.volume_multiplier, self.volume_softmax = "softmax", 1.0, True


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=lambda s: [int(x) for x in s.split(",")], default=[8, 32])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-model", action="store_true", help="skip the whole-module rows")
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

    emit(f"# feature convolution Conv2d({CIN}, 32, 1) on B x {N} maps of {HM}^2; {args.repeats} repeats x {args.calls} calls "
         f"after 10 warm-up calls, paths alternating in one process; median us per call (device, HIP events), spread = "
         f"range of the repeats")
    emit(f"# {torch.cuda.get_device_name(0)}; of 8 TB/s = (bytes / 8 TB/s) / time; of MFMA floor = (tiles x {CIN // 2} x "
         f"{MFMA_CYCLES} cycles / {SIMDS} SIMDs / 2.4 GHz) / time")
    torch.manual_seed(0)
    net = Net().eval()
    conv = net.process_features[0]
    w4, b = conv.weight.detach().to(dev), conv.bias.detach().to(dev)
    w2 = w4.view(32, CIN).contiguous()
    bf16, f32 = torch.bfloat16, torch.float32
    with torch.no_grad():
        emit(f"{'row':<12} {'B':>3} {'kernel us':>10} {'spread':>7} {'MB':>7} {'of 8 TB/s':>9} {'of MFMA floor':>13} "
             f"{'torch us':>9} {'spread':>7} {'torch channels_last us':>22} {'spread':>7} {'best torch / kernel':>19} "
             f"{'difference - spreads':>20}")
        for B in args.frames:
            M = B * N
            x32 = torch.randn((M, CIN, HM, HM), generator=torch.Generator().manual_seed(B)).to(dev)
            for name, di, do in (("f32->f32", f32, f32), ("f32->bf16", f32, bf16), ("bf16->bf16", bf16, bf16)):
                x = x32.to(di)
                xc = x.contiguous(memory_format=torch.channels_last)
                wt, bt = w4.to(di), b.to(di)
                wc = wt.contiguous(memory_format=torch.channels_last)

                def stock(xi, wi):
                    y = F.conv2d(xi, wi, bt)
                    return y if y.dtype == do else y.to(do)
                r = alternate({"ours": lambda: model.feature_conv(x, w2, b, out_dtype=do),
                               "torch": lambda: stock(x, wt), "torch_cl": lambda: stock(xc, wc)})
                us, spr = r["ours"]
                px = M * HM * HM
                nbytes = px * (CIN * x.element_size() + 32 * (4 if do is f32 else 2)) + 32 * CIN * 4
                floor_us = (px / 32) * (CIN // 2) * MFMA_CYCLES / SIMDS / CLOCK_HZ * 1e6
                best = min(("torch", "torch_cl"), key=lambda k: r[k][0])
                emit(f"{name:<12} {B:>3} {us:>10.1f} {spr:>7.1f} {nbytes / 1e6:>7.1f} {nbytes / HBM_BYTES_PER_S * 1e6 / us:>9.3f} "
                     f"{floor_us / us:>13.3f} {r['torch'][0]:>9.1f} {r['torch'][1]:>7.1f} {r['torch_cl'][0]:>22.1f} "
                     f"{r['torch_cl'][1]:>7.1f} {r[best][0] / us:>19.3f} {r[best][0] - us - r[best][1] - spr:>20.1f}")
                del x, xc
            del x32
            torch.cuda.empty_cache()

        if not args.no_model:
            evs = {"bf16": model.VolumetricEval.from_reference(net, device=dev, feature_dtype=bf16),
                   "f32": model.VolumetricEval.from_reference(net, device=dev, feature_dtype=f32)}
            v2veval = evs["bf16"].v2v
            emit(f"# whole module at {V}^3, J = {J}, softmax aggregation, cuboids: VolumetricEval.forward against "
                 f"F.conv2d (f32), .to(bfloat16), unproject_channels_last, V2VEval.forward")
            emit(f"{'row':<34} {'B':>3} {'us':>11} {'spread':>9}")
            for B in args.frames:
                vb = synth.volumetric_batch(B, n_views=N, channels=8, heatmap=HM, volume=V, seed=1)
                feats = torch.randn((B, N, CIN, HM, HM), generator=torch.Generator().manual_seed(B)).to(dev)
                proj, cub = vb.proj.to(dev), vb.cuboids(dev)

                def four_calls():
                    f = F.conv2d(feats.view(B * N, CIN, HM, HM), w4, b).view(B, N, 32, HM, HM).to(bf16)
                    return v2veval(v2v.unproject_channels_last(f, proj, cub, "softmax"), cub, 1.0, True)
                r = alternate({"VolumetricEval, bf16 features": lambda: evs["bf16"](feats, proj, cub),
                               "VolumetricEval, f32 features": lambda: evs["f32"](feats, proj, cub),
                               "four calls (F.conv2d, cast, ...)": four_calls})
                for key, (us, spr) in r.items():
                    emit(f"{key:<34} {B:>3} {us:>11.1f} {spr:>9.1f}")
                base = r["four calls (F.conv2d, cast, ...)"]
                ours = r["VolumetricEval, bf16 features"]
                emit(f"difference four calls - VolumetricEval (bf16) {base[0] - ours[0]:>10.1f} us; sum of the two spreads "
                     f"{base[1] + ours[1]:>8.1f} us")
                del feats
                torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
