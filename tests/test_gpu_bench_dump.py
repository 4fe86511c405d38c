"""A plain `bench.py --gpus 1 --steps K --warmup W` run: it times K steps and prints the line
without the legs that moved behind --full, and `--dump-outputs DIR` writes what its last
timed step computed — the same arrays this process computes from the same seeded frames."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_lean_and_dumps_its_last_step(tmp_path, device):
    import torch

    import bench
    from mvn_rocm import op, synth
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--settle", "0", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["metric"] == bench.METRIC and line["unit"] == "frames/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f32" and line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["ms_per_step"] > 0
    # value and ms_per_step are the same measurement: 8 frames per step
    assert line["value"] == pytest.approx(8 / (line["ms_per_step"] * 1e-3), rel=1e-9)
    # nothing that moved behind --full ran
    for k in ("cpu_baseline", "parity", "telemetry", "secondary", "other_precision", "config1", "in_kernel_coords",
              "config4", "config5"):
        assert line[k] is None, k
    assert "measured_copy_gbps" not in line["roofline"]

    files = sorted(os.listdir(out))
    assert files == ["joints.npy", "softargmax_volumes.npy", "unprojected_volume.npy"]
    got = {f[:-4]: np.load(out / f) for f in files}
    assert all(a.dtype == np.float32 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 * 2 ** 20

    c = bench._configs()["2"]
    vb = synth.volumetric_batch(c["frames"], n_views=c["views"], channels=c["channels"], heatmap=c["heatmap"],
                                volume=c["volume"], dtype=c["dtype"], device=device, seed=0, first_frame=0)
    vol = op.unproject_heatmaps(vb.features, vb.proj, vb.coords, "softmax", precision="exact")
    xyz, sm = op.integrate_tensor_3d_with_coordinates(vol[:, :c["joints"]], vb.coords, True)
    assert got["joints"].shape == (c["frames"], c["joints"], 3)
    assert np.array_equal(got["joints"], xyz.cpu().numpy())
    for name, t in (("unprojected_volume", vol), ("softargmax_volumes", sm)):
        idx = np.sort(np.random.default_rng(0).integers(0, t.numel(), bench.DUMP_SAMPLE))
        ref = t.reshape(-1)[torch.from_numpy(idx).to(device)].cpu().numpy()
        assert got[name].shape == (bench.DUMP_SAMPLE,)
        assert np.isfinite(got[name]).all() and np.array_equal(got[name], ref), name
