"""Device time of the algebraic chain from heatmaps: the one-launch kernel against the composition
of the existing ops (mvn_rocm.multiview.triangulate_from_heatmaps, fused=True / fused=False).

    python tools/time_algebraic.py [--batches 1,8,16,64,256] [--maps off|on|both] [--repeats 7] [--calls 100]
                                   [--parent-lib PATH/libmvn_hip.so] [--out FILE]

bench.py::run_config1's protocol per measurement: 10 warm-up calls, then HIP events around
`calls` back-to-back calls.  The two paths alternate in one process, `repeats` measurements
each; the table gives the median and the range (max - min) of the repeats, the spread.  Shapes:
N = 4, J = 17, 96 x 96 float32 maps, multiplier 100, with and without the returned maps.

--parent-lib: also A/B mvn_softargmax2d and mvn_dlt of this build against another build of the
library (the parent commit's), called through the C ABI, outputs compared bitwise.

For kernel durations run the same script under `rocprofv3 --kernel-trace --stats -- python ...`
(with --batches 1 --maps off --repeats 1 --calls 20 to keep the trace small and one shape per run)."""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "learnable-triangulation-pytorch_amd"))
import torch  # noqa: E402

from mvn_rocm import _lib, multiview, synth  # noqa: E402


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


def alternate(fns, repeats, calls):
    """{name: [us per call] * repeats}, the functions taking turns."""
    res = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            res[name].append(measure(fn, calls))
    return res


def summary(v):
    return statistics.median(v), max(v) - min(v)


def time_paths(args, dev, emit):
    emit(f"# algebraic chain from heatmaps, N=4 J=17 96x96 f32, multiplier 100; {args.repeats} repeats x {args.calls} "
         f"calls, alternating; median us per call (device, HIP events), spread = range of the repeats")
    emit(f"# {torch.cuda.get_device_name(0)}")
    emit(f"{'B':>4} {'B*J':>5} {'maps':>5} {'unfused us':>11} {'spread':>7} {'fused us':>9} {'spread':>7} {'fused/unfused':>13}  verdict")
    for B in args.batches:
        ab = synth.algebraic_batch(B, 4, 17, seed=0)
        proj = ab.proj.to(dev)
        hm = torch.randn((B, 4, 17, 96, 96), generator=torch.Generator().manual_seed(1)).to(dev)
        conf = (torch.rand((B, 4, 17), generator=torch.Generator().manual_seed(2)) + 0.1).to(dev)
        for maps in args.maps:
            def call(fused):
                return multiview.triangulate_from_heatmaps(hm, proj, conf, image_shape=(384, 384),
                                                           heatmap_multiplier=100.0, return_heatmaps=maps, fused=fused)
            same = all(torch.equal(a, b) for a, b in zip(call(True), call(False)) if a is not None)
            res = alternate({"unfused": lambda: call(False), "fused": lambda: call(True)}, args.repeats, args.calls)
            (mu, su), (mf, sf) = summary(res["unfused"]), summary(res["fused"])
            spread = max(su, sf)
            verdict = "fused faster" if mf < mu - spread else ("fused slower" if mf > mu + spread else "within spread")
            emit(f"{B:>4} {B * 17:>5} {'yes' if maps else 'no':>5} {mu:>11.1f} {su:>7.1f} {mf:>9.1f} {sf:>7.1f} "
                 f"{mf / mu:>13.2f}  {verdict}{'' if same else '  OUTPUTS DIFFER'}")


def ab_parent(args, dev, emit):
    """mvn_softargmax2d and mvn_dlt of this build against --parent-lib, through the C ABI."""
    libs = {"parent": ctypes.CDLL(os.path.abspath(args.parent_lib)), "this": _lib.load()}
    for lib in libs.values():
        for name in ("mvn_softargmax2d", "mvn_dlt"):
            getattr(lib, name).restype, getattr(lib, name).argtypes = _lib.SIGNATURES[name]
    stream = torch.cuda.current_stream().cuda_stream
    emit("")
    emit(f"# refactored kernels, this build against {os.path.basename(args.parent_lib)} (the parent commit's); "
         f"median us per call, spread = range of {args.repeats} repeats")
    emit(f"{'kernel':28} {'shape':22} {'parent us':>10} {'spread':>7} {'this us':>8} {'spread':>7}  same bits")
    for B in (1, 64):
        ab = synth.algebraic_batch(B, 4, 17, seed=0)
        P, pts, conf = ab.proj.to(dev), ab.points.to(dev), ab.confidences.to(dev)
        hm = torch.randn((B * 4, 17, 96, 96), generator=torch.Generator().manual_seed(1)).to(dev)
        hm3 = torch.randn((B * 4, 17, 50, 50), generator=torch.Generator().manual_seed(1)).to(dev)
        for kname, src, softmax, maps in (("softargmax2d_reg softmax", hm, 1, False), ("softargmax2d_reg softmax+maps", hm, 1, True),
                                          ("softargmax2d_reg relu+maps", hm, 0, True), ("softargmax2d softmax+maps", hm3, 1, True)):
            outs = {k: (torch.empty((src.shape[0], 17, 2), device=dev), torch.empty_like(src)) for k in libs}

            def run(k):
                xy, m = outs[k]
                code = libs[k].mvn_softargmax2d(src.data_ptr(), 0, 100.0, softmax, xy.data_ptr(),
                                                m.data_ptr() if maps else None, 0, src.shape[0], 17, src.shape[2],
                                                src.shape[3], stream)
                assert code == 0, code
            res = alternate({k: (lambda k=k: run(k)) for k in libs}, args.repeats, args.calls)
            same = torch.equal(outs["parent"][0], outs["this"][0]) and (not maps or torch.equal(outs["parent"][1], outs["this"][1]))
            (mp, sp), (mt, st) = summary(res["parent"]), summary(res["this"])
            emit(f"{kname:28} {str(tuple(src.shape)):22} {mp:>10.2f} {sp:>7.2f} {mt:>8.2f} {st:>7.2f}  {same}")
        outs = {k: torch.empty((B, 17, 3), device=dev) for k in libs}

        def run_dlt(k):
            code = libs[k].mvn_dlt(P.data_ptr(), pts.data_ptr(), conf.data_ptr(), outs[k].data_ptr(), B, 4, 17, stream)
            assert code == 0, code
        res = alternate({k: (lambda k=k: run_dlt(k)) for k in libs}, args.repeats, args.calls)
        (mp, sp), (mt, st) = summary(res["parent"]), summary(res["this"])
        emit(f"{'dlt_kernel':28} {str((B, 4, 17)):22} {mp:>10.2f} {sp:>7.2f} {mt:>8.2f} {st:>7.2f}  "
             f"{torch.equal(outs['parent'], outs['this'])}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=lambda s: [int(x) for x in s.split(",")], default=[1, 8, 16, 64, 256])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--maps", type=lambda s: {"off": [False], "on": [True], "both": [False, True]}[s], default=[False, True],
                    help="return_heatmaps: off, on or both (default)")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    time_paths(args, dev, emit)
    if args.parent_lib:
        ab_parent(args, dev, emit)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
