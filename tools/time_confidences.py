"""Device time of the backbone's confidence head on the kernels (csrc/confidence_head.hip,
``confidence.ConfidenceHeadEval``) against the same ``GlobalAveragePoolingHead`` run by torch on the same box, and of
``model.AlgebraicModelEval`` with every switch on the kernels against the model in torch.

    python tools/time_confidences.py [--frames 8,32] [--repeats 5] [--calls 20] [--out FILE]

The method of tools/time_trunk.py and tools/time_stem.py: per measurement 10 warm-up calls, then HIP events around
`calls` back-to-back calls; the paths alternate in one process, `repeats` measurements each; the table gives the
median and the range (max - min) of the repeats.

The head reads ``layer4``'s output behind B frames x 4 views of 384^2 images: (4 B, 2048, 12, 12) bfloat16 in
channels_last memory format, what the kernel trunk returns.  Rows of the head alone, n = 17 and n = 32 outputs:
  kernels              ConfidenceHeadEval: three launches;
  f32 cast + torch f32 what ``confidences="torch"`` runs behind the kernel trunk today: the cast of the maps to float32
                       and the float32 module;
  torch bf16 cl        the module in bfloat16 channels_last on the maps as they are.
Rows of the launches alone: the first stage (2048 -> 512, 12 x 12 -> 6 x 6) and the second (512 -> 256, 6 x 6 -> 3 x 3)
and the tail; per stage the fraction of the dense bf16 rate (2.5 PFLOP/s) on the 2 * 9 * Cin * Cout multiply-adds per
convolution pixel.
Rows from the images to the joints (ResNet-152 stages of tools/time_trunk.py, the stem of tools/time_stem.py, the
deconv head of tools/time_deconv_head.py, a head with n = 17 and ``use_confidences``): AlgebraicModelEval with
``trunk``, ``stem`` and ``confidences`` on the kernels against the backbone as torch modules in float32 and in
bfloat16 channels_last, each followed by the same ``multiview.triangulate_from_heatmaps``.  A row is won if the faster
torch path is slower by more than the sum of the two ranges (the rule of DESIGN.md §4.16)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "learnable-triangulation-pytorch_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
from torch import nn  # noqa: E402

from mvn_rocm import confidence, model, multiview, synth  # noqa: E402
from time_deconv_head import Head, init  # noqa: E402
from time_stem import IMAGE, Stem  # noqa: E402
from time_trunk import DENSE_BF16, N, stages  # noqa: E402
from time_v2v_res3d import measure  # noqa: E402

C4, MAP, J = 2048, IMAGE // 32, 17


class GapHead(nn.Module):
    """GlobalAveragePoolingHead as the reference's PoseResNet builds it."""

    def __init__(self, cin, n):
        super().__init__()
        self.features = nn.Sequential(
            nn.Conv2d(cin, 512, 3, stride=1, padding=1), nn.BatchNorm2d(512), nn.MaxPool2d(2), nn.ReLU(inplace=True),
            nn.Conv2d(512, 256, 3, stride=1, padding=1), nn.BatchNorm2d(256), nn.MaxPool2d(2), nn.ReLU(inplace=True))
        self.head = nn.Sequential(nn.Linear(256, 512), nn.ReLU(inplace=True), nn.Linear(512, 256), nn.ReLU(inplace=True),
                                  nn.Linear(256, n), nn.Sigmoid())

    def forward(self, x):
        x = self.features(x)
        return self.head(x.view(x.shape[0], x.shape[1], -1).mean(dim=-1))


class PoseNet(nn.Module):
    """The reference's PoseResNet-152 by attribute names, with the algebraic confidence head."""

    def __init__(self):
        super().__init__()
        stem, head = Stem(), Head()
        self.conv1, self.bn1, self.relu, self.maxpool = stem.conv1, stem.bn1, stem.relu, stem.maxpool
        self.layer1, self.layer2, self.layer3, self.layer4 = stages()
        self.alg_confidences = GapHead(C4, J)
        self.deconv_layers, self.final_layer = head.deconv_layers, head.final_layer

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.final_layer(self.deconv_layers(x)), self.alg_confidences(x)


class AlgebraicNet(nn.Module):
    """The attributes of AlgebraicTriangulationNet that AlgebraicModelEval reads."""

    def __init__(self, backbone):
        super().__init__()
        self.backbone, self.use_confidences, self.heatmap_softmax, self.heatmap_multiplier = backbone, True, True, 100.0


def bf16_copy(module, make):
    twin = init(make()).to(dtype=torch.bfloat16)
    twin.load_state_dict({k: v.to(torch.bfloat16) if v.is_floating_point() else v for k, v in module.state_dict().items()})
    return twin.to(device=next(module.parameters()).device, memory_format=torch.channels_last)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=lambda s: [int(x) for x in s.split(",")], default=[8, 32])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-model", action="store_true", help="skip the images-to-joints rows")
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

    def alternate(fns, calls):
        res = {k: [] for k in fns}
        for _ in range(args.repeats):
            for k, fn in fns.items():
                res[k].append(measure(fn, calls))
        return {k: (statistics.median(v), max(v) - min(v)) for k, v in res.items()}

    bf16, cl = torch.bfloat16, torch.channels_last
    emit(f"# confidence head (2 x [3x3 conv + BN + 2x2 max pool + ReLU], mean, 3 Linear, sigmoid) on (B x {N}, {C4}, {MAP}, {MAP}) "
         f"bf16 channels_last maps; {args.repeats} repeats x {args.calls} calls after 10 warm-up calls, paths alternating in one "
         f"process; median us per call (device, HIP events), spread = range of the repeats")
    emit(f"# {torch.cuda.get_device_name(0)}; of dense bf16 = (FLOP / 2.5 PFLOP/s) / time; best = the faster torch path; "
         f"difference - spreads = best torch - kernel - both spreads: positive means the kernel wins by more than the sum of "
         f"the two ranges")
    emit(f"{'row':<40} {'B':>3} {'us':>10} {'spread':>8} {'of dense bf16':>13} {'best torch / kernel':>19} {'difference - spreads':>20}")

    def rows(B, r, kernel, flops=None):
        torch_rows = [k for k in r if k not in kernel]
        best = min(torch_rows, key=lambda k: r[k][0]) if torch_rows else None
        for k, (us, spr) in r.items():
            frac = f"{flops[k] / DENSE_BF16 * 1e6 / us:>13.4f}" if flops and k in flops else f"{'':>13}"
            tail = f"{r[best][0] / us:>19.3f} {r[best][0] - us - r[best][1] - spr:>20.1f}" if best and k in kernel else ""
            emit(f"{k:<40} {B:>3} {us:>10.1f} {spr:>8.1f} {frac} {tail}")

    with torch.no_grad():
        for n in (17, 32):
            head32 = init(GapHead(C4, n)).to(dev)
            head16 = bf16_copy(head32, lambda: GapHead(C4, n))
            ours = confidence.ConfidenceHeadEval.from_reference(head32, device=dev)
            p = ours.params
            for B in args.frames:
                M = B * N
                x = torch.randn((M, C4, MAP, MAP), generator=torch.Generator().manual_seed(B)).abs().to(dev)
                x = x.to(bf16).contiguous(memory_format=cl)
                r = alternate({f"head n={n}: kernels": lambda: ours(x),
                               f"head n={n}: f32 cast + torch f32": lambda: head32(x.to(torch.float32)),
                               f"head n={n}: torch bf16 cl": lambda: head16(x)}, args.calls)
                rows(B, r, (f"head n={n}: kernels",))
                if n != 17:
                    continue
                x_cl = x.permute(0, 2, 3, 1)
                h1 = confidence.conv3x3_pool(x_cl, *p.conv1)
                h2 = confidence.conv3x3_pool(h1, *p.conv2, out_dtype=torch.float32)
                fns = {"stage 1 (2048 -> 512)": lambda: confidence.conv3x3_pool(x_cl, *p.conv1),
                       "stage 2 (512 -> 256)": lambda: confidence.conv3x3_pool(h1, *p.conv2, out_dtype=torch.float32)}
                flops = {"stage 1 (2048 -> 512)": M * MAP * MAP * 2 * 9 * C4 * 512,
                         "stage 2 (512 -> 256)": M * (MAP // 2) ** 2 * 2 * 9 * 512 * 256}
                fns["tail (256-512-256-17)"] = lambda: confidence.confidence_tail(h2, p.tail)
                r = alternate(fns, args.calls)
                rows(B, r, tuple(fns), flops)
                del x, x_cl, h1, h2
                torch.cuda.empty_cache()
        if not args.no_model:
            net32 = init(PoseNet()).to(dev)
            net16 = bf16_copy(net32, PoseNet)
            ours = model.AlgebraicModelEval.from_reference(AlgebraicNet(net32), device=dev, trunk="kernels", stem="kernels",
                                                           confidences="kernels")
            assert not any(isinstance(m, (nn.Conv2d, nn.Linear, nn.ConvTranspose2d)) for m in ours.modules())

            def torch_model(net, images, proj):
                hm, conf = net(images)
                return multiview.triangulate_from_heatmaps(hm, proj, conf, image_shape=(IMAGE, IMAGE), heatmap_multiplier=100.0)

            for B in args.frames:
                images = torch.randn((B, N, 3, IMAGE, IMAGE), generator=torch.Generator().manual_seed(B)).to(dev)
                flat = images.view(B * N, 3, IMAGE, IMAGE)
                proj = synth.algebraic_batch(B, N, J, seed=1).proj.float().to(dev)
                r = alternate({"model: AlgebraicModelEval on kernels": lambda: ours(images, proj),
                               "model: torch f32": lambda: torch_model(net32, flat, proj),
                               "model: torch bf16 cl": lambda: torch_model(net16, flat.to(bf16).contiguous(memory_format=cl), proj)},
                              max(2, args.calls // 4))
                rows(B, r, ("model: AlgebraicModelEval on kernels",))
                del images, flat
                torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
