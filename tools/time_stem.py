"""Device time of the ResNet stem in one launch (csrc/stem.hip, ``resnet.StemEval``) against the same ``conv1, bn1,
relu, maxpool`` run by torch on the same box.

    python tools/time_stem.py [--frames 8,32] [--repeats 5] [--calls 20] [--out FILE]

The method of tools/time_trunk.py: per measurement 10 warm-up calls, then HIP events around `calls` back-to-back
calls; the paths alternate in one process, `repeats` measurements each; the table gives the median and the range
(max - min) of the repeats.

The images are B frames x 4 views of 3 x 384^2 f32.  Rows of the stem alone, each from the f32 images to a
64 x 96^2 map:
  kernel            StemEval: one launch, bf16 channels-last out;
  torch f32 + cast  the modules in f32, default memory format, then the cast-and-permute pass of
                    ``TrunkEval.channels_last`` (what ``stem="torch"`` runs in front of the kernel trunk);
  torch bf16 cl     the modules in bf16 channels_last, the cast of the images included (the kernel's time includes
                    its own rounding of them).
Rows from the images to the head's features (ResNet-152 stages of tools/time_trunk.py, the deconv head of
tools/time_deconv_head.py): stem + trunk + head on the kernels, the torch f32 stem + cast in front of the kernel trunk
and head (``trunk="kernels", stem="torch"``), and the two torch paths end to end.  The kernel wins a row if the
faster torch path is slower by more than the sum of the two ranges (the rule of DESIGN.md §4.16).  Per stem row:
the fraction of the dense bf16 rate (2.5 PFLOP/s) on the 2 * 147 * 64 multiply-adds per convolution pixel, and of
8 TB/s on the algorithmic bytes (the f32 images read once, the bf16 map written once, the weights read once)."""
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
from time_trunk import DENSE_BF16, HBM_BYTES_PER_S, N, stages  # noqa: E402
from time_v2v_res3d import measure  # noqa: E402

IMAGE = 384


class Stem(nn.Module):
    """conv1, bn1, relu, maxpool as the reference's PoseResNet builds them."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)

    def forward(self, x):
        return self.maxpool(self.relu(self.bn1(self.conv1(x))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=lambda s: [int(x) for x in s.split(",")], default=[8, 32])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-model", action="store_true", help="skip the stem + trunk + head rows")
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
    emit(f"# ResNet stem (7x7 stride-2 conv + BN + ReLU + 3x3 stride-2 max pool) on B x {N} f32 images of 3 x {IMAGE}^2; "
         f"{args.repeats} repeats x {args.calls} calls after 10 warm-up calls, paths alternating in one process; median us per "
         f"call (device, HIP events), spread = range of the repeats")
    emit(f"# {torch.cuda.get_device_name(0)}; of dense bf16 = (FLOP / 2.5 PFLOP/s) / time; of 8 TB/s = (bytes / 8 TB/s) / time; "
         f"best = the faster torch path; difference - spreads = best torch - kernel - both spreads: positive means the kernel "
         f"wins by more than the sum of the two ranges")
    stem32 = init(Stem()).to(dev)
    stem16 = init(Stem()).to(device=dev, dtype=bf16)
    stem16.load_state_dict({k: v.to(bf16) if v.is_floating_point() else v for k, v in stem32.state_dict().items()})
    stem16 = stem16.to(memory_format=cl)
    with torch.no_grad():
        ours = resnet.StemEval.from_reference(stem32, device=dev)

        def torch_cast(x):
            h = stem32(x).permute(0, 2, 3, 1)
            return torch.empty(h.shape, dtype=bf16, device=h.device).copy_(h)

        def torch_cl(x):
            return stem16(x.to(bf16).contiguous(memory_format=cl))

        if not args.no_model:
            net32 = init(stages()).to(dev)
            net16 = init(stages()).to(device=dev, dtype=bf16)
            net16.load_state_dict({k: v.to(bf16) if v.is_floating_point() else v for k, v in net32.state_dict().items()})
            net16 = net16.to(memory_format=cl)
            head32 = init(Head()).to(dev)
            head16 = init(Head()).to(device=dev, dtype=bf16, memory_format=cl)
            blocks = [resnet.BottleneckCL.from_reference(b, device=dev) for layer in net32 for b in layer]
            head = backbone.DeconvHeadEval.from_reference(head32, device=dev, heatmaps=False)

            def behind(h):
                for b in blocks:
                    h = b(h)
                return head(h.permute(0, 3, 1, 2))

        emit(f"{'row':<34} {'B':>3} {'us':>10} {'spread':>8} {'of dense bf16':>13} {'of 8 TB/s':>9} {'best torch / kernel':>19} "
             f"{'difference - spreads':>20}")

        def rows(B, names, r, kernel, flop=None, nbytes=None):
            best = min((k for k in names if k not in kernel), key=lambda k: r[k][0])
            for k in names:
                us, spr = r[k]
                frac = f"{flop / DENSE_BF16 * 1e6 / us:>13.4f} {nbytes / HBM_BYTES_PER_S * 1e6 / us:>9.3f}" if flop else f"{'':>13} {'':>9}"
                tail = f"{r[best][0] / us:>19.3f} {r[best][0] - us - r[best][1] - spr:>20.1f}" if k in kernel else ""
                emit(f"{k:<34} {B:>3} {us:>10.1f} {spr:>8.1f} {frac} {tail}")

        for B in args.frames:
            M = B * N
            x = torch.randn((M, 3, IMAGE, IMAGE), generator=torch.Generator().manual_seed(B)).to(dev)
            hc, hp = IMAGE // 2, IMAGE // 4
            flop = M * hc * hc * 2 * 147 * 64
            nbytes = M * (3 * IMAGE * IMAGE * 4 + hp * hp * 64 * 2) + 64 * 192 * 2
            r = alternate({"stem: kernel": lambda: ours(x), "stem: torch f32 + cast": lambda: torch_cast(x),
                           "stem: torch bf16 cl": lambda: torch_cl(x)})
            rows(B, list(r), r, ("stem: kernel",), flop, nbytes)
            if not args.no_model:
                r = alternate({"model: kernel stem, trunk, head": lambda: behind(ours(x)),
                               "model: torch f32 stem, kernels": lambda: behind(torch_cast(x)),
                               "model: torch f32": lambda: head32.deconv_layers(net32(stem32(x))),
                               "model: torch bf16 cl": lambda: head16.deconv_layers(net16(torch_cl(x)))})
                rows(B, list(r), r, ("model: kernel stem, trunk, head", "model: torch f32 stem, kernels"))
            del x
            torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
