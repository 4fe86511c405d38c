"""Time triangulate_ransac_batch at config 1's shape (8 frames, 4 views, 17 joints) with 10 shared
view pairs, one outlier view per point displaced by 80-250 px: hypotheses + inlier DLT alone
(direct_optimization=False) and with the Huber refinement, next to the confidence-weighted DLT
and the reprojection-error op on the same inputs.  hipEvents around 100 back-to-back calls after
50 warm-up calls; the median of 21 such batches, per call.
    python tools/time_ransac.py"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "learnable-triangulation-pytorch_amd"))
import torch  # noqa: E402

from mvn_rocm import _ops, multiview, synth  # noqa: E402

dev = torch.device("cuda:0")
B, N, J, PAIRS = 8, 4, 17, 10
ab = synth.algebraic_batch(B, N, J, seed=0)
g = torch.Generator().manual_seed(0)
pts = ab.points.clone()
view = torch.randint(0, N, (B, J), generator=g)
ang = torch.rand(B, J, generator=g) * 6.2831853
mag = 80.0 + 170.0 * torch.rand(B, J, generator=g)
shift = torch.stack([mag * torch.cos(ang), mag * torch.sin(ang)], dim=-1)
pts[torch.arange(B)[:, None], view, torch.arange(J)[None, :]] += shift
proj, pts, conf = ab.proj.to(dev), pts.to(dev), ab.confidences.to(dev)
pairs = multiview.random_view_pairs(1, 1, N, PAIRS, "cpu", g)[0, 0].to(dev)


def timed(fn, warmup=50, batch=100, batches=21):
    """Per-call time in us: hipEvents around `batch` back-to-back calls, median / min / max of `batches`."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(batches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(batch):
            fn()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / batch)
    return statistics.median(us), min(us), max(us)


xyz, inl = multiview.triangulate_ransac_batch(proj, pts, view_pairs=pairs)
print(f"{torch.cuda.get_device_name(0)}; B={B} N={N} J={J}, {PAIRS} shared pairs {pairs.tolist()}; "
      f"inlier counts {sorted(set(inl.sum(-1).flatten().tolist()))}", flush=True)
eps = 15.0
rows = (
    ("DLT, confidence-weighted (mvn_dlt)", lambda: multiview.triangulate_batch_of_points(proj, pts, conf)),
    ("RANSAC op, direct_optimization=False", lambda: _ops.ransac.eager(proj, pts, pairs, eps, False)),
    ("RANSAC op, direct_optimization=True", lambda: _ops.ransac.eager(proj, pts, pairs, eps, True)),
    ("triangulate_ransac_batch, False", lambda: multiview.triangulate_ransac_batch(
        proj, pts, view_pairs=pairs, direct_optimization=False)),
    ("triangulate_ransac_batch, True", lambda: multiview.triangulate_ransac_batch(
        proj, pts, view_pairs=pairs, direct_optimization=True)),
    ("reprojection error (B, J, N)", lambda: multiview.calc_reprojection_error_matrix(xyz, pts, proj)),
)
for name, fn in rows:
    med, lo, hi = timed(fn)
    print(f"{name:38s} {med:7.1f} us per call (min {lo:.1f}, max {hi:.1f} over 21 batches of 100)", flush=True)
print("op rows: one kernel launch + three output allocations; triangulate_ransac_batch adds the unpacking of "
      "the bit masks into a (B, J, N) bool tensor (small torch kernels).  Back-to-back calls on one stream: "
      "the larger of the host's enqueue time and the kernel's duration.")
