"""``confidence.ConfidenceHeadEval`` and the ``confidences="kernels"`` switch of ``BackboneEval`` and
``VolumetricModelEval`` on the GPU, on the stand-ins of tests/confidence_kit.py: heads in the
reference's form, a backbone whose 64 x 96 images leave 8 x 12 maps of 256 channels, M = 3 images."""
import copy
import functools

import pytest
import torch
from torch import nn

from confidence_kit import IMAGE, head_reference, head_stage_bounds, real_head, small_head, stand_in_backbone, stand_in_volumetric_model
from v2v_kit import assert_same_bits, bf16r

pytestmark = pytest.mark.gpu

M = 3
HEADS = {"small": (small_head, (3, 64, 5, 6)), "real": (real_head, (2, 2048, 4, 4))}


@functools.lru_cache(maxsize=None)
def head_input(name):
    """Non-negative bf16-exact maps, as behind the trunk's last ReLU."""
    shape = HEADS[name][1]
    return bf16r(torch.randn(shape, generator=torch.Generator().manual_seed(sum(shape))).abs())


@functools.lru_cache(maxsize=None)
def images():
    return torch.randn(M, 3, *IMAGE, generator=torch.Generator().manual_seed(81))


def by_hand(module, x):
    """The three launches made one by one on a channels-last bfloat16 copy of x."""
    from mvn_rocm import confidence
    p = module.params
    h = x.permute(0, 2, 3, 1).to(torch.bfloat16).contiguous()
    h = confidence.conv3x3_pool(h, *p.conv1, out_dtype=torch.bfloat16)
    assert h.dtype == torch.bfloat16
    h = confidence.conv3x3_pool(h, *p.conv2, out_dtype=torch.float32)
    assert h.dtype == torch.float32
    return confidence.confidence_tail(h, p.tail, sigmoid=True)


@pytest.mark.parametrize("name", HEADS)
def test_forward_is_the_three_launches(device, name):
    from mvn_rocm import confidence
    module = confidence.ConfidenceHeadEval.from_reference(HEADS[name][0](), device=device)
    x = head_input(name).to(device)
    got = module(x)                                                  # float32 NCHW: the cast-and-permute pass
    n = module.widths[3]
    assert tuple(got.shape) == (x.shape[0], n) and got.dtype == torch.float32
    assert_same_bits(got, by_hand(module, x))
    assert_same_bits(module(x.bfloat16()), got)                      # bfloat16 NCHW
    assert_same_bits(module(x.bfloat16().contiguous(memory_format=torch.channels_last)), got)
    assert bool(((got > 0) & (got < 1)).all())


def test_a_bfloat16_channels_last_input_is_read_without_a_copy(device, monkeypatch):
    from mvn_rocm import confidence
    module = confidence.ConfidenceHeadEval.from_reference(small_head(), device=device)
    x_cl = head_input("small").to(device).bfloat16().permute(0, 2, 3, 1).contiguous()     # what TrunkEval's kernels write
    x = x_cl.permute(0, 3, 1, 2)                                                          # and what it returns
    seen = []
    launch = confidence.conv3x3_pool

    def spy(x_in, *args, **kw):
        seen.append(x_in)
        return launch(x_in, *args, **kw)
    monkeypatch.setattr(confidence, "conv3x3_pool", spy)
    module(x)
    module(head_input("small").to(device))
    monkeypatch.undo()
    assert len(seen) == 4
    assert seen[0].data_ptr() == x_cl.data_ptr() and tuple(seen[0].shape) == tuple(x_cl.shape)
    assert seen[2].data_ptr() != x_cl.data_ptr() and seen[2].dtype == torch.bfloat16 and seen[2].is_contiguous()


@pytest.mark.parametrize("name", HEADS)
def test_within_the_carried_bound_of_the_float64_restatement(device, name):
    """The head launch by launch against the float64 restatement with bf16-rounded convolution operands, each
    launch on the input it really read (confidence_kit.head_stage_bounds): a bound carried end to end has to let
    every bf16 rounding of the first stage flip and grows past 1 on the way to the logits, so it could not fail;
    these three are a few f32 ulps of their sums (printed).  The module's output is the third launch's, bit for
    bit.  The distances to the end-to-end restatement and to the f32 torch module are printed, not asserted."""
    from mvn_rocm import confidence
    head = HEADS[name][0]()
    x = head_input(name)
    module = confidence.ConfidenceHeadEval.from_reference(head, device=device)
    p = module.params
    xd = x.to(device)
    h1 = confidence.conv3x3_pool(xd.permute(0, 2, 3, 1).to(torch.bfloat16).contiguous(), *p.conv1, out_dtype=torch.bfloat16)
    h2 = confidence.conv3x3_pool(h1, *p.conv2, out_dtype=torch.float32)
    out = confidence.confidence_tail(h2, p.tail, sigmoid=True)
    assert_same_bits(module(xd), out)
    got = [h1.cpu().float().permute(0, 3, 1, 2), h2.cpu().permute(0, 3, 1, 2), out.cpu()]
    for (what, ref, bound), g in zip(head_stage_bounds(head, x, got[0], got[1]), got):
        frac = float(((g.double() - ref).abs() / bound).max())
        print(f"ConfidenceHeadEval {name}, {what}: worst |got - ref| / bound = {frac:.4f} (bound up to {float(bound.max()):.3e})")
        assert float(bound.max()) < (1.0 if what == "confidences" else float("inf")) and frac <= 1.0
    ref, _ = head_reference(head, x)
    with torch.no_grad():
        f32 = head(x)
    print(f"ConfidenceHeadEval {name}: max |got - end-to-end float64 restatement| = {float((got[2].double() - ref).abs().max()):.3e}; "
          f"max |got - f32 torch module| = {float((got[2] - f32).abs().max()):.3e}")


# ----------------------------------------------------------------------------- BackboneEval
def on_device(device):
    return copy.deepcopy(stand_in_backbone()).to(device), images().to(device)


@pytest.mark.parametrize("trunk, stem", (("kernels", "kernels"), ("torch", "torch")), ids=("kernel_trunk", "torch_trunk"))
def test_backbone_confidences_are_the_head_modules_on_the_trunks_output(device, trunk, stem):
    from mvn_rocm import backbone, confidence
    net, x = on_device(device)
    be = backbone.BackboneEval.from_reference(net, device=device, trunk=trunk, stem=stem, confidences="kernels")
    bt = backbone.BackboneEval.from_reference(net, device=device, trunk=trunk, stem=stem)
    assert isinstance(be.alg_confidences, confidence.ConfidenceHeadEval) and isinstance(be.vol_confidences, confidence.ConfidenceHeadEval)
    assert bt.alg_confidences is net.alg_confidences and bt.vol_confidences is net.vol_confidences
    if trunk == "kernels":
        assert not any(isinstance(m, (nn.Conv2d, nn.Linear)) for m in be.modules())
    seen = []
    hook = be.trunk.register_forward_hook(lambda mod, args, out: seen.append(out))
    with torch.no_grad():
        hm, f, alg, vol = be(x)
        hook.remove()
        x4, = seen                                                   # the very maps this run's heads read
        alg_w = confidence.ConfidenceHeadEval.from_reference(net.alg_confidences, device=device)(x4)
        vol_w = confidence.ConfidenceHeadEval.from_reference(net.vol_confidences, device=device)(x4)
        if trunk == "kernels":
            assert_same_bits(x4, be.trunk(x))                        # the kernel trunk repeats itself bit for bit
            hm_t, f_t, alg_t, vol_t = bt(x)
        else:
            # torch's own convolutions need not repeat their bits from one call to the next (the first run of this
            # trunk in a process differed from the later ones on the MI355X): compare behind the same maps
            (hm_t, f_t), alg_t, vol_t = bt.head(x4), bt.alg_confidences(x4), bt.vol_confidences(x4)
    assert tuple(x4.shape) == (M, 256, IMAGE[0] // 8, IMAGE[1] // 8)
    assert tuple(alg.shape) == (M, 17) and tuple(vol.shape) == (M, 32) and alg.dtype == vol.dtype == torch.float32
    assert_same_bits(alg, alg_w)
    assert_same_bits(vol, vol_w)
    assert_same_bits(hm, hm_t)                                       # the rest of the backbone does not notice
    assert_same_bits(f, f_t)
    # the torch heads on the same maps, printed and not asserted: the bound is test_within_the_carried_bound's
    print(f"BackboneEval trunk={trunk}: max |kernels - torch| alg {float((alg - alg_t).abs().max()):.3e}, "
          f"vol {float((vol - vol_t).abs().max()):.3e}")


# ----------------------------------------------------------------------------- VolumetricModelEval
def test_volumetric_model_with_conf_aggregation_reads_the_kernel_confidences(device):
    """B = 1, N = 3, V = 32, 'conf' aggregation: the model equals ``VolumetricEval.from_projected`` fed the
    separately computed features and ``ConfidenceHeadEval`` confidences, bit for bit."""
    from mvn_rocm import backbone, confidence, model, synth
    B, N, V = 1, 3, 32
    net = copy.deepcopy(stand_in_volumetric_model()).to(device)
    x = images().to(device).view(B, N, 3, *IMAGE)
    vb = synth.volumetric_batch(B, n_views=N, channels=8, heatmap=IMAGE[0], volume=V, seed=3)
    proj, coords = vb.proj.to(device), vb.cuboids(device)
    kw = dict(trunk="kernels", stem="kernels", confidences="kernels")
    me = model.VolumetricModelEval.from_reference(net, device=device, **kw)
    assert me.volumetric.volume_aggregation_method == "conf"
    assert not any(isinstance(m, (nn.Conv2d, nn.Linear)) for m in me.backbone.modules())
    be = backbone.BackboneEval.from_reference(net.backbone, device=device, heatmaps=False,
                                              process_features=net.process_features, trunk="kernels", stem="kernels")
    ev = model.VolumetricEval.from_reference(net, device=device)
    with torch.no_grad():
        got = me(x, proj, coords)
        _, f, _, _ = be(x.view(B * N, 3, *IMAGE))
        vc = confidence.ConfidenceHeadEval.from_reference(net.backbone.vol_confidences, device=device)(be.trunk(x.view(B * N, 3, *IMAGE)))
        want = ev.from_projected(f.view(B, N, *f.shape[1:]), proj, coords, vc.view(B, N, 32))
    assert len(got) == len(want) == 4
    for g, w in zip(got, want):
        assert_same_bits(g, w)
    assert tuple(got[0].shape) == (B, 5, 3) and bool(torch.isfinite(got[0]).all())
    assert_same_bits(got[3], vc.view(B, N, 32))
