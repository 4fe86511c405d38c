"""install() rebinds the reference's hot-path module attributes (no GPU needed: only the
library load and the rebinding are exercised)."""
import types

from mvn_rocm import install, multiview, op


def test_install_rebinds_every_hot_path_function():
    ref_op = types.SimpleNamespace(unproject_heatmaps=object(), integrate_tensor_3d_with_coordinates=object(),
                                   integrate_tensor_2d=object())
    ref_mv = types.SimpleNamespace(triangulate_batch_of_points=object())
    before = dict(vars(ref_op), **vars(ref_mv))
    prev = install(ref_op, ref_mv)
    assert prev == before
    assert ref_op.unproject_heatmaps is op.unproject_heatmaps
    assert ref_op.integrate_tensor_3d_with_coordinates is op.integrate_tensor_3d_with_coordinates
    assert ref_op.integrate_tensor_2d is op.integrate_tensor_2d
    assert ref_mv.triangulate_batch_of_points is multiview.triangulate_batch_of_points


# a stand-in for the reference's package layout: the hot-path functions live in mvn/utils/op.py and
# mvn/utils/multiview.py, and mvn/models/triangulation.py reaches them by attribute lookup on those
# two modules (`from mvn.utils import op, multiview`), which is what makes install() a drop-in
MVN_TREE = {
    "mvn/__init__.py": "",
    "mvn/utils/__init__.py": "",
    "mvn/models/__init__.py": "",
    "mvn/utils/op.py": "".join(f"def {n}(*a, **k):\n    raise AssertionError('{n} was not rebound')\n\n\n"
                               for n in ("integrate_tensor_2d", "integrate_tensor_3d_with_coordinates",
                                         "unproject_heatmaps")),
    "mvn/utils/multiview.py": "def triangulate_batch_of_points(*a, **k):\n"
                              "    raise AssertionError('triangulate_batch_of_points was not rebound')\n",
    "mvn/models/triangulation.py": "from mvn.utils import op, multiview\n\n\n"
                                   "def call_sites():\n"
                                   "    return (op.unproject_heatmaps, op.integrate_tensor_3d_with_coordinates,\n"
                                   "            op.integrate_tensor_2d, multiview.triangulate_batch_of_points)\n",
}


def test_install_on_an_importable_mvn_package(tmp_path):
    """install() with no arguments imports `mvn.utils.op` and `mvn.utils.multiview` itself and
    rebinds them in place.  On a package laid out as the reference (MVN_TREE), the names the
    model module resolves at its call sites (op.unproject_heatmaps,
    op.integrate_tensor_3d_with_coordinates, op.integrate_tensor_2d,
    multiview.triangulate_batch_of_points) are mvn_rocm's afterwards, and install() returns the
    package's own functions.  Run in a subprocess so that `mvn` never enters this test process's
    modules."""
    import os
    import subprocess
    import sys
    for rel, text in MVN_TREE.items():
        f = tmp_path / rel
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_text(text)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = f"""
import sys
sys.dont_write_bytecode = True
sys.path.insert(0, {str(tmp_path)!r})
sys.path.insert(0, {os.path.join(root, "learnable-triangulation-pytorch_amd")!r})
from mvn.models import triangulation as T
import mvn_rocm
from mvn_rocm import op, multiview
prev = mvn_rocm.install()
assert T.op.unproject_heatmaps is op.unproject_heatmaps
assert T.op.integrate_tensor_3d_with_coordinates is op.integrate_tensor_3d_with_coordinates
assert T.op.integrate_tensor_2d is op.integrate_tensor_2d
assert T.multiview.triangulate_batch_of_points is multiview.triangulate_batch_of_points
assert T.call_sites() == (op.unproject_heatmaps, op.integrate_tensor_3d_with_coordinates, op.integrate_tensor_2d,
                          multiview.triangulate_batch_of_points)
assert sorted(prev) == ["integrate_tensor_2d", "integrate_tensor_3d_with_coordinates", "triangulate_batch_of_points",
                        "unproject_heatmaps"]
assert prev["unproject_heatmaps"].__module__ == "mvn.utils.op"
assert prev["integrate_tensor_3d_with_coordinates"].__module__ == "mvn.utils.op"
assert prev["integrate_tensor_2d"].__module__ == "mvn.utils.op"
assert prev["triangulate_batch_of_points"].__module__ == "mvn.utils.multiview"
print("ok")
"""
    r = subprocess.run([sys.executable, "-B", "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]
