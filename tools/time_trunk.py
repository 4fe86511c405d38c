"""Device time of the backbone's ResNet trunk on kernels (csrc/bottleneck.hip, mvn_rocm/resnet.py) against the
same ``layer1`` .. ``layer4`` modules run by torch on the same box.

    python tools/time_trunk.py [--frames 8,32] [--repeats 5] [--calls 20] [--out FILE]

The method of tools/time_deconv_head.py: per measurement 10 warm-up calls, then HIP events around `calls`
back-to-back calls; the paths alternate in one process, `repeats` measurements each; the table gives the
median and the range (max - min) of the repeats.

The network is ResNet-152's stages (3, 8, 36, 3 Bottleneck blocks of 64, 128, 256, 512 middle channels) built
from torch.nn with random weights, on B frames x 4 views of 384^2 images: layer1 reads the stem's 64 x 96^2
maps, layer4 writes 2048 x 12^2.  The kernels read and write channels-last bf16, three launches per block;
torch runs the same modules in f32 with the default memory format and in bf16 channels_last (inputs prepared
outside the timed region); the faster of the two is the comparison.  Rows: each stage on its own input, the
four stages in a row, and the stages followed by the deconv head (DeconvHeadEval, features only, against
torch's deconv_layers).  Per kernel row: the fraction of the dense bf16 rate (2.5 PFLOP/s) on the row's
multiply-adds, and of 8 TB/s on the algorithmic bytes (every launch reads its inputs once, writes its output
once and reads its weights once; the trunk + head row repeats the trunk's bytes)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "learnable-triangulation-pytorch_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
from torch import nn  # noqa: E402

from mvn_rocm import backbone, resnet  # noqa: E402
from time_deconv_head import Head, init  # noqa: E402
from time_v2v_res3d import measure  # noqa: E402

N, H1 = 4, 96
STAGES = ((64, 3, 1), (128, 8, 2), (256, 36, 2), (512, 3, 2))        # (middle channels, blocks, stride)
DENSE_BF16, HBM_BYTES_PER_S = 2.5e15, 8e12


class Bottleneck(nn.Module):
    """1x1, 3x3 carrying the stride, 1x1 to four times the width, each with a BatchNorm; the residual through
    ``downsample`` where the shape changes."""

    def __init__(self, inplanes, planes, stride=1):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv2d(inplanes, planes, 1, bias=False), nn.BatchNorm2d(planes)
        self.conv2, self.bn2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False), nn.BatchNorm2d(planes)
        self.conv3, self.bn3 = nn.Conv2d(planes, 4 * planes, 1, bias=False), nn.BatchNorm2d(4 * planes)
        self.relu = nn.ReLU(inplace=True)
        self.downsample, self.stride = None, stride
        if stride != 1 or inplanes != 4 * planes:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, 4 * planes, 1, stride=stride, bias=False),
                                            nn.BatchNorm2d(4 * planes))

    def forward(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        return self.relu(out + (x if self.downsample is None else self.downsample(x)))


def stages():
    layers, cin = [], 64
    for planes, blocks, stride in STAGES:
        layers.append(nn.Sequential(Bottleneck(cin, planes, stride), *(Bottleneck(4 * planes, planes) for _ in range(blocks - 1))))
        cin = 4 * planes
    return nn.Sequential(*layers)


def block_cost(block, M, h):
    """(multiply-add FLOP, algorithmic bytes, output extent) of one block's three launches on M maps of h x h."""
    cin, mid, cout, s = block.conv1.in_channels, block.conv1.out_channels, block.conv3.out_channels, block.stride
    ho = (h - 1) // s + 1
    p_in, p_out = M * h * h, M * ho * ho
    flop = 2 * p_in * cin * mid + 2 * p_out * 9 * mid * mid + 2 * p_out * mid * cout
    nbytes = 2 * (p_in * cin + p_in * mid + cin * mid) + 2 * (p_in * mid + p_out * mid + 9 * mid * mid)
    nbytes += 2 * (p_out * mid + p_out * cout + mid * cout)
    if block.downsample is not None:
        flop += 2 * p_out * cin * cout
        nbytes += 2 * (p_in * cin + cin * cout)
    else:
        nbytes += 2 * p_out * cout
    return flop, nbytes, ho


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=lambda s: [int(x) for x in s.split(",")], default=[8, 32])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
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
    emit(f"# ResNet-152 trunk: layer1 .. layer4 = {', '.join(str(b) for _, b, _ in STAGES)} Bottleneck blocks on B x {N} maps of "
         f"64 x {H1}^2 (384^2 images behind the stem); {args.repeats} repeats x {args.calls} calls after 10 warm-up calls, paths "
         f"alternating in one process; median us per call (device, HIP events), spread = range of the repeats")
    emit(f"# {torch.cuda.get_device_name(0)}; of dense bf16 = (FLOP / 2.5 PFLOP/s) / time; of 8 TB/s = (bytes / 8 TB/s) / time; "
         f"torch = the same modules in f32 (default format) and in bf16 channels_last, best = the faster; difference - spreads = "
         f"best torch - kernel - both spreads: positive means the kernels win by more than the sum of the two ranges")
    net32 = init(stages()).to(dev)
    net16 = init(stages()).to(device=dev, dtype=bf16)
    net16.load_state_dict({k: v.to(bf16) for k, v in net32.state_dict().items()})
    net16 = net16.to(memory_format=cl)
    head32 = init(Head()).to(dev)
    head16 = init(Head()).to(device=dev, dtype=bf16, memory_format=cl)
    with torch.no_grad():
        ours = [[resnet.BottleneckCL.from_reference(b, device=dev) for b in layer] for layer in net32]
        head = backbone.DeconvHeadEval.from_reference(head32, device=dev, heatmaps=False)
        emit(f"{'row':<22} {'B':>3} {'kernel us':>10} {'spread':>7} {'GFLOP':>8} {'of dense bf16':>13} {'MB':>8} {'of 8 TB/s':>9} "
             f"{'torch f32 us':>12} {'spread':>7} {'torch bf16 cl us':>16} {'spread':>7} {'best torch / kernel':>19} "
             f"{'difference - spreads':>20}")

        def row(name, B, r, flop, nbytes):
            us, spr = r["ours"]
            best = min(("torch", "torch_cl"), key=lambda k: r[k][0])
            emit(f"{name:<22} {B:>3} {us:>10.1f} {spr:>7.1f} {flop / 1e9:>8.1f} {flop / DENSE_BF16 * 1e6 / us:>13.3f} "
                 f"{nbytes / 1e6:>8.1f} {nbytes / HBM_BYTES_PER_S * 1e6 / us:>9.3f} {r['torch'][0]:>12.1f} {r['torch'][1]:>7.1f} "
                 f"{r['torch_cl'][0]:>16.1f} {r['torch_cl'][1]:>7.1f} {r[best][0] / us:>19.3f} "
                 f"{r[best][0] - us - r[best][1] - spr:>20.1f}")

        def run(blocks, x):
            for b in blocks:
                x = b(x)
            return x

        for B in args.frames:
            M = B * N
            g = torch.Generator().manual_seed(B)
            h, cin, total_flop, total_bytes = H1, 64, 0, 0
            for i, layer in enumerate(net32):
                x32 = torch.randn((M, cin, h, h), generator=g).relu_().to(dev)
                x16 = x32.to(bf16).contiguous(memory_format=cl)
                xk = x16.permute(0, 2, 3, 1).contiguous()
                flop = nbytes = 0
                hh = h
                for b in layer:
                    f, nb, hh = block_cost(b, M, hh)
                    flop, nbytes = flop + f, nbytes + nb
                r = alternate({"ours": lambda: run(ours[i], xk), "torch": lambda: layer(x32), "torch_cl": lambda: net16[i](x16)})
                row(f"layer{i + 1} ({cin} x {h}^2)", B, r, flop, nbytes)
                total_flop, total_bytes = total_flop + flop, total_bytes + nbytes
                h, cin = hh, layer[-1].conv3.out_channels
                del x32, x16, xk
                torch.cuda.empty_cache()
            x32 = torch.randn((M, 64, H1, H1), generator=g).relu_().to(dev)
            x16 = x32.to(bf16).contiguous(memory_format=cl)
            xk = x16.permute(0, 2, 3, 1).contiguous()
            every = [b for layer in ours for b in layer]
            r = alternate({"ours": lambda: run(every, xk), "torch": lambda: net32(x32), "torch_cl": lambda: net16(x16)})
            row("trunk", B, r, total_flop, total_bytes)
            head_flop = sum(M * (2 * hh_) ** 2 * 2 * 4 * c * 256 for c, hh_ in ((2048, 12), (256, 24), (256, 48)))
            r = alternate({"ours": lambda: head(run(every, xk).permute(0, 3, 1, 2)),
                           "torch": lambda: head32.deconv_layers(net32(x32)),
                           "torch_cl": lambda: head16.deconv_layers(net16(x16))})
            row("trunk + head", B, r, total_flop + head_flop, total_bytes)
            del x32, x16, xk
            torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
