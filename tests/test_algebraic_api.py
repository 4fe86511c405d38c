"""Host side of the one-call algebraic triangulation -- no GPU needed: the C ABI's argument
checks return before any HIP call, the Python wrapper asserts what the reference asserts, and
the custom op traces under fake tensors."""
import ctypes
import os

import pytest
import torch
from torch.fx.experimental.proxy_tensor import make_fx

ARG, SHAPE, DTYPE = -1, -2, -3
F32, BF16 = 0, 1


@pytest.fixture(scope="module")
def lib():
    from mvn_rocm import _lib
    return _lib.load()


def _call(lib, **kw):
    a = dict(heatmaps=1, dtype=F32, multiplier=100.0, softmax=1, proj=1, conf=None, scale_x=4.0, scale_y=4.0,
             out_xyz=1, out_kp2d=1, out_xy=1, out_conf=1, out_maps=None, maps_dtype=F32, B=2, N=4, J=17, H=96, W=96)
    a.update(kw)
    return lib.mvn_algebraic_triangulate(a["heatmaps"], a["dtype"], a["multiplier"], a["softmax"], a["proj"],
                                         a["conf"], a["scale_x"], a["scale_y"], a["out_xyz"], a["out_kp2d"],
                                         a["out_xy"], a["out_conf"], a["out_maps"], a["maps_dtype"], a["B"], a["N"],
                                         a["J"], a["H"], a["W"], None)


@pytest.mark.parametrize("name", ["heatmaps", "proj", "out_xyz", "out_kp2d", "out_xy", "out_conf"])
def test_null_required_pointers(lib, name):
    assert _call(lib, **{name: None}) == ARG


@pytest.mark.parametrize("softmax", [2, -1])
def test_bad_softmax_flag(lib, softmax):
    assert _call(lib, softmax=softmax) == ARG


@pytest.mark.parametrize("kw", [dict(B=0), dict(N=0), dict(J=0), dict(H=0), dict(W=-1), dict(B=-1), dict(N=33),
                                dict(B=1 << 16, J=1 << 15), dict(B=1 << 14, N=32, J=1 << 14),
                                dict(H=1 << 16, W=1 << 15)])
def test_bad_shapes(lib, kw):
    assert _call(lib, **kw) == SHAPE


@pytest.mark.parametrize("pair", [(F32, BF16), (2, F32), (F32, 2), (BF16, 7), (-1, -1)])
def test_bad_dtype_pairs(lib, pair):
    assert _call(lib, dtype=pair[0], maps_dtype=pair[1]) == DTYPE
    assert _call(lib, dtype=pair[0], maps_dtype=pair[1], out_maps=1) == DTYPE


def test_header_declares_and_library_exports_the_entry_point(lib):
    from conftest import ROOT
    from mvn_rocm import _lib
    header = open(os.path.join(ROOT, "include", "mvn_hip.h")).read()
    assert "int mvn_algebraic_triangulate(" in header
    assert "mvn_algebraic_triangulate" in _lib.SIGNATURES
    assert isinstance(lib.mvn_algebraic_triangulate, ctypes._CFuncPtr)


def _targets(gm):
    return {str(n.target) for n in gm.graph.nodes if n.op == "call_function"}


@pytest.mark.parametrize("layout", ["bnjhw", "flat"])
@pytest.mark.parametrize("dtype,out_dtype,want", [(torch.float32, None, torch.float32),
                                                  (torch.bfloat16, None, torch.bfloat16),
                                                  (torch.bfloat16, torch.float32, torch.float32)])
def test_custom_op_traces_under_fake_tensors(layout, dtype, out_dtype, want):
    from mvn_rocm import multiview
    B, N, J, H, W = 2, 4, 5, 24, 32
    hm = torch.randn(B, N, J, H, W).to(dtype)
    conf = torch.rand(B, N, J)
    if layout == "flat":
        hm, conf = hm.reshape(B * N, J, H, W), conf.reshape(B * N, J)
    proj = torch.randn(B, N, 3, 4)

    def f(hm, proj, conf):
        return multiview.triangulate_from_heatmaps(hm, proj, conf, image_shape=(96, 128), heatmap_multiplier=100.0,
                                                   out_dtype=out_dtype)

    gm = make_fx(f, tracing_mode="fake")(hm, proj, conf)
    assert "mvn_rocm.algebraic_triangulate.default" in _targets(gm)
    out = [n for n in gm.graph.nodes if n.op == "output"][0].args[0]
    xyz, kp2d, maps, cn = (n.meta["val"] for n in out)
    assert (tuple(xyz.shape), xyz.dtype) == ((B, J, 3), torch.float32)
    assert (tuple(kp2d.shape), kp2d.dtype) == ((B, N, J, 2), torch.float32)
    assert (tuple(maps.shape), maps.dtype) == ((B, N, J, H, W), want)
    assert (tuple(cn.shape), cn.dtype) == ((B, N, J), torch.float32)


def test_trace_without_maps_and_without_confidences():
    from mvn_rocm import multiview
    hm, proj = torch.randn(1, 3, 2, 16, 16), torch.randn(1, 3, 3, 4)

    def f(h, p):
        xyz, kp2d, maps, cn = multiview.triangulate_from_heatmaps(h, p, image_shape=(64, 64), return_heatmaps=False)
        assert maps is None
        return xyz, cn

    gm = make_fx(f, tracing_mode="fake")(hm, proj)
    assert "mvn_rocm.algebraic_triangulate.default" in _targets(gm)
    xyz, cn = (n.meta["val"] for n in [n for n in gm.graph.nodes if n.op == "output"][0].args[0])
    assert tuple(xyz.shape) == (1, 2, 3) and tuple(cn.shape) == (1, 3, 2)


def test_no_cpu_fallback():
    from mvn_rocm import multiview
    hm, proj, conf = torch.randn(1, 4, 3, 16, 16), torch.randn(1, 4, 3, 4), torch.rand(1, 4, 3)
    for fused in (None, True, False):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            multiview.triangulate_from_heatmaps(hm, proj, conf, image_shape=(64, 64), fused=fused)


def test_wrapper_asserts_what_the_reference_asserts():
    from mvn_rocm import multiview
    proj = torch.randn(2, 4, 3, 4)
    with pytest.raises(AssertionError):                       # multiview.py:143
        multiview.triangulate_from_heatmaps(torch.randn(2, 3, 5, 16, 16), proj, image_shape=(64, 64))
    with pytest.raises(AssertionError):
        multiview.triangulate_from_heatmaps(torch.randn(7, 5, 16, 16), proj, image_shape=(64, 64))
    with pytest.raises(AssertionError):
        multiview.triangulate_from_heatmaps(torch.randn(2, 4, 5, 16, 16), proj, torch.rand(2, 3, 5), image_shape=(64, 64))


def test_unsupported_dtypes_raise_type_error():
    from mvn_rocm import multiview
    proj = torch.randn(1, 4, 3, 4)
    with pytest.raises(TypeError):
        multiview.triangulate_from_heatmaps(torch.randn(1, 4, 5, 16, 16).half(), proj, image_shape=(64, 64))
    with pytest.raises(TypeError):
        multiview.triangulate_from_heatmaps(torch.randn(1, 4, 5, 16, 16).double(), proj, image_shape=(64, 64))
    with pytest.raises(TypeError):
        multiview.triangulate_from_heatmaps(torch.randn(1, 4, 5, 16, 16), proj, image_shape=(64, 64),
                                            out_dtype=torch.bfloat16)
    with pytest.raises(TypeError):
        multiview.triangulate_from_heatmaps(torch.randn(1, 4, 5, 16, 16), proj, image_shape=(64, 64),
                                            out_dtype=torch.float16)
