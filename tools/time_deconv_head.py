"""Device time of the backbone's deconv head on kernels (csrc/deconv_head.hip, mvn_rocm/backbone.py)
against the reference's own ``deconv_layers`` + ``final_layer`` modules run by torch on the same box.

    python tools/time_deconv_head.py [--frames 8,32] [--repeats 5] [--calls 20] [--out FILE] [--project]

The method of tools/time_feature_conv.py: per measurement 10 warm-up calls, then HIP events around
`calls` back-to-back calls; the paths alternate in one process, `repeats` measurements each; the
table gives the median and the range (max - min) of the repeats.

Layer rows: B frames x 4 views; layer 1 is ConvTranspose2d(2048, 256, 4, 2, 1) + BN + ReLU on 12^2
maps, layers 2 and 3 the same from 256 channels on 24^2 and 48^2.  The kernel reads channels-last
bf16 and writes channels-last bf16 (layers 1, 2) or NCHW bf16 (layer 3).  torch runs the same three
modules in f32 with the default memory format and in bf16 channels_last (inputs prepared outside the
timed region); the faster of the two is the comparison.  Per kernel row: the fraction of the dense
bf16 rate (2.5 PFLOP/s) on the layer's 2 x 4 x Cin x 256 FLOP per output pixel, and of 8 TB/s on the
algorithmic bytes (x once, y once, the weight once).

Head rows: DeconvHeadEval.forward on layer4's (4 B, 2048, 12, 12) output, features only and with the
heatmaps (J = 17), from an f32 input in the default format and from a bf16 channels_last input,
against torch's deconv_layers (and final_layer) in its two forms.

--project prints another table instead: the last layer with the volumetric model's
process_features (a Conv2d(256, 32, 1)) behind it, as the parent's two launches (deconv4s2 to NCHW,
then model.feature_conv) against the one launch of deconv4s2_project, for bf16 and f32 features, and
the whole head (bf16 channels_last in) followed by feature_conv against the head with ``project``."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "learnable-triangulation-pytorch_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
from torch import nn  # noqa: E402

from mvn_rocm import backbone, model  # noqa: E402
from time_v2v_res3d import measure  # noqa: E402

N, C4, H4, COUT, J = 4, 2048, 12, 256, 17
DENSE_BF16, HBM_BYTES_PER_S = 2.5e15, 8e12


class Head(nn.Module):
    """deconv_layers and final_layer as the reference's PoseResNet builds them (ResNet-152 widths)."""

    def __init__(self):
        super().__init__()
        layers, cin = [], C4
        for _ in range(3):
            layers += [nn.ConvTranspose2d(cin, COUT, 4, stride=2, padding=1, output_padding=0, bias=False),
                       nn.BatchNorm2d(COUT), nn.ReLU(inplace=True)]
            cin = COUT
        self.deconv_layers = nn.Sequential(*layers)
        self.final_layer = nn.Conv2d(COUT, J, 1)


def init(module):
    torch.manual_seed(0)
    for c in module.modules():
        if isinstance(c, (nn.Conv2d, nn.ConvTranspose2d)):
            nn.init.xavier_normal_(c.weight)
        elif isinstance(c, nn.BatchNorm2d):
            c.running_mean.normal_(0, 0.2)
            c.running_var.uniform_(0.75, 1.25)
    for p in module.parameters():
        p.requires_grad_(False)
    return module.eval()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=lambda s: [int(x) for x in s.split(",")], default=[8, 32])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--project", action="store_true", help="the fused projection against the two launches")
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

    bf16, cl = torch.bfloat16, torch.channels_last
    if args.project:
        project_table(args, dev, emit, alternate)
        if out:
            out.close()
        return
    emit(f"# deconv head: 3 x (ConvTranspose2d(Cin, {COUT}, 4, 2, 1) + BN + ReLU) on B x {N} maps of {C4} x {H4}^2, final_layer to "
         f"J = {J}; {args.repeats} repeats x {args.calls} calls after 10 warm-up calls, paths alternating in one process; "
         f"median us per call (device, HIP events), spread = range of the repeats")
    emit(f"# {torch.cuda.get_device_name(0)}; of dense bf16 = (FLOP / 2.5 PFLOP/s) / time; of 8 TB/s = (bytes / 8 TB/s) / time; "
         f"torch = the same modules in f32 (default format) and in bf16 channels_last, best = the faster")
    net = init(Head())
    net32 = net.to(dev)
    net16 = init(Head()).to(device=dev, dtype=bf16, memory_format=cl)
    net16.load_state_dict({k: v.to(bf16) for k, v in net32.state_dict().items()})
    net16 = net16.to(memory_format=cl)
    with torch.no_grad():
        params = [backbone.fold_deconv_block(net.deconv_layers[3 * i], net.deconv_layers[3 * i + 1], device=dev) for i in range(3)]
        heads = {True: backbone.DeconvHeadEval.from_reference(net, device=dev, heatmaps=True),
                 False: backbone.DeconvHeadEval.from_reference(net, device=dev, heatmaps=False)}
        emit(f"{'row':<22} {'B':>3} {'kernel us':>10} {'spread':>7} {'GFLOP':>7} {'of dense bf16':>13} {'MB':>7} {'of 8 TB/s':>9} "
             f"{'torch f32 us':>12} {'spread':>7} {'torch bf16 cl us':>16} {'spread':>7} {'best torch / kernel':>19} "
             f"{'difference - spreads':>20}")

        def row(name, B, r, flop, nbytes):
            us, spr = r["ours"]
            best = min(("torch", "torch_cl"), key=lambda k: r[k][0])
            emit(f"{name:<22} {B:>3} {us:>10.1f} {spr:>7.1f} {flop / 1e9:>7.1f} {flop / DENSE_BF16 * 1e6 / us:>13.3f} "
                 f"{nbytes / 1e6:>7.1f} {nbytes / HBM_BYTES_PER_S * 1e6 / us:>9.3f} {r['torch'][0]:>12.1f} {r['torch'][1]:>7.1f} "
                 f"{r['torch_cl'][0]:>16.1f} {r['torch_cl'][1]:>7.1f} {r[best][0] / us:>19.3f} "
                 f"{r[best][0] - us - r[best][1] - spr:>20.1f}")

        for B in args.frames:
            M = B * N
            g = torch.Generator().manual_seed(B)
            total_flop = 0
            for i, (cin, h) in enumerate(((C4, H4), (COUT, 2 * H4), (COUT, 4 * H4))):
                x32 = torch.randn((M, cin, h, h), generator=g).to(dev)
                x16 = x32.to(bf16).contiguous(memory_format=cl)
                xk = x16.permute(0, 2, 3, 1).contiguous()
                m32, m16 = net32.deconv_layers[3 * i:3 * i + 3], net16.deconv_layers[3 * i:3 * i + 3]
                layout = "nchw" if i == 2 else "cl"
                r = alternate({"ours": lambda: backbone.deconv4s2(xk, params[i], layout),
                               "torch": lambda: m32(x32), "torch_cl": lambda: m16(x16)})
                flop = M * (2 * h) ** 2 * 2 * 4 * cin * COUT
                total_flop += flop
                nbytes = M * h * h * cin * 2 + M * (2 * h) ** 2 * COUT * 2 + cin * COUT * 16 * 2
                row(f"layer {i + 1} ({cin} x {h}^2)", B, r, flop, nbytes)
                del x32, x16, xk
            x32 = torch.randn((M, C4, H4, H4), generator=g).to(dev)
            x16 = x32.to(bf16).contiguous(memory_format=cl)
            nb_feat = M * H4 * H4 * C4 * 2 + M * (8 * H4) ** 2 * COUT * 2
            for hm in (False, True):
                t32 = (lambda: net32.final_layer(net32.deconv_layers(x32))) if hm else (lambda: net32.deconv_layers(x32))
                t16 = (lambda: net16.final_layer(net16.deconv_layers(x16))) if hm else (lambda: net16.deconv_layers(x16))
                what = "head + heatmaps" if hm else "head, features"
                r = alternate({"ours": lambda: heads[hm](x32), "torch": t32, "torch_cl": t16})
                row(f"{what}, f32 in", B, r, total_flop, nb_feat)
                r = alternate({"ours": lambda: heads[hm](x16), "torch": t32, "torch_cl": t16})
                row(f"{what}, bf16 cl in", B, r, total_flop, nb_feat)
            del x32, x16
            torch.cuda.empty_cache()
    if out:
        out.close()


def project_table(args, dev, emit, alternate):
    """Layer 3 + process_features, unfused (two launches) against fused (one), and the head both ways."""
    bf16, cl = torch.bfloat16, torch.channels_last
    emit(f"# last deconv layer ({COUT} x {4 * H4}^2 -> {COUT} x {8 * H4}^2) + Conv2d({COUT}, 32, 1) on B x {N} maps: unfused = deconv4s2 "
         f"(NCHW) then feature_conv, fused = deconv4s2_project; head = DeconvHeadEval from a bf16 channels_last layer4 output; "
         f"{args.repeats} repeats x {args.calls} calls after 10 warm-up calls, paths alternating in one process; median us per "
         f"call (device, HIP events), spread = range of the repeats")
    emit(f"# {torch.cuda.get_device_name(0)}; difference - spreads = unfused - fused - both spreads: positive means the fused "
         f"launch wins by more than the sum of the two ranges")
    net = init(Head())
    pf = init(nn.Sequential(nn.Conv2d(COUT, 32, 1)))
    with torch.no_grad():
        params = [backbone.fold_deconv_block(net.deconv_layers[3 * i], net.deconv_layers[3 * i + 1], device=dev) for i in range(3)]
        pw, pb = pf[0].weight.detach().reshape(32, COUT).to(dev), pf[0].bias.detach().to(dev)
        proj = backbone.pack_projection(pw, pb, device=dev)
        emit(f"{'row':<28} {'B':>3} {'features':>8} {'unfused us':>10} {'spread':>7} {'fused us':>9} {'spread':>7} "
             f"{'unfused / fused':>15} {'difference - spreads':>20}")

        def row(name, B, dt, r):
            (u, us), (f, fs) = r["unfused"], r["fused"]
            emit(f"{name:<28} {B:>3} {str(dt).replace('torch.', ''):>8} {u:>10.1f} {us:>7.1f} {f:>9.1f} {fs:>7.1f} {u / f:>15.3f} "
                 f"{u - f - us - fs:>20.1f}")

        for B in args.frames:
            M = B * N
            g = torch.Generator().manual_seed(B)
            xk = torch.randn((M, 4 * H4, 4 * H4, COUT), generator=g).to(dev).to(bf16)
            x16 = torch.randn((M, C4, H4, H4), generator=g).to(dev).to(bf16).contiguous(memory_format=cl)
            r = alternate({"unfused": lambda: backbone.deconv4s2(xk, params[2], "nchw"),
                           "fused": lambda: backbone.deconv4s2(xk, params[2], "nchw")})
            row("layer 3 alone, twice", B, bf16, r)
            for dt in (bf16, torch.float32):
                r = alternate({"unfused": lambda: model.feature_conv(backbone.deconv4s2(xk, params[2], "nchw", dt), pw, pb,
                                                                     out_dtype=dt),
                               "fused": lambda: backbone.deconv4s2_project(xk, params[2], proj, dt)})
                row("layer 3 + process_features", B, dt, r)
            for dt in (bf16, torch.float32):
                plain = backbone.DeconvHeadEval.from_reference(net, device=dev, feature_dtype=dt, heatmaps=False)
                fused = backbone.DeconvHeadEval.from_reference(net, device=dev, feature_dtype=dt, heatmaps=False,
                                                               process_features=pf)
                r = alternate({"unfused": lambda: model.feature_conv(plain(x16)[1], pw, pb, out_dtype=dt),
                               "fused": lambda: fused(x16)[1]})
                row("head + process_features", B, dt, r)
            del xk, x16
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
