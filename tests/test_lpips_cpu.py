"""CPU: the LPIPS fixture g28 (tools/make_golden_lpips.py, the real reference on synthetic weights) against the float64
restatement tests/lpips_ref.py, and the host side of dsml_thesis_amd.lpips: key layout, factory names, refusals."""
import numpy as np
import pytest
import torch

import lpips_ref as R
from conftest import golden


@pytest.fixture(autouse=True)
def _grad_mode_on():
    """some modules of the suite switch autograd off process-wide when they are imported; these tests differentiate"""
    with torch.enable_grad():
        yield


@pytest.fixture(scope="module")
def g28():
    return golden("g28_lpips.npz")


@pytest.fixture(scope="module")
def weights(g28):
    from dsml_thesis_amd import synth
    return synth.lpips_state_dict(int(g28["weight_seed"]))


def _rel(got, ref):
    ref = torch.as_tensor(ref).double()
    return ((torch.as_tensor(got).double() - ref).abs().max() / ref.abs().max()).item()


@pytest.mark.parametrize("tag", ["a", "b"])
def test_float64_restatement_reproduces_the_reference_fixture(g28, weights, tag):
    """lpips_ref in float64 against the float64 twin of the reference, under the stored bounds (4 x the fp32 reference's own
    deviation); the fixture's own conditions are checked again."""
    x, y = torch.from_numpy(g28[f"{tag}_input"]), torch.from_numpy(g28[f"{tag}_target"])
    assert x.shape[0] == 2 and x.shape[1] == 3 and x.abs().max() <= 1 and y.abs().max() <= 1
    for img in (x, y):
        for f in R.features(img, weights):
            assert ((f ** 2).sum(dim=1) > 0).all(), "no all-zero vector at any tap: the reference's gradient is NaN-free"
    val, gi, gt = R.value_and_grads(x, y, weights)
    for name, got, tol in (("val", val, "tol_val"), ("grad_target", gt, "tol_grad_target"), ("grad_input", gi, "tol_grad_input")):
        e, bound = _rel(got, g28[f"{tag}_{name}_f64"]), float(g28[f"{tag}_{tol}"])
        print(f"[{tag}] {name}: float64 restatement {e:.3e} / bound {bound:.3e}")
        assert e <= bound, f"[{tag}] {name}: {e:.3e} > {bound:.3e}"
        assert np.isfinite(g28[f"{tag}_{name}"]).all() and np.isfinite(g28[f"{tag}_{name}_f64"]).all()
        assert 0 < bound < 1e-4
    # the fp32 reference sits inside its own bound by construction (a quarter of it)
    assert _rel(g28[f"{tag}_val"], g28[f"{tag}_val_f64"]) <= float(g28[f"{tag}_tol_val"]) / 3.9


def test_closed_form_layer_gradient_is_autograd_away_from_zero_vectors():
    """layer_bwd, the closed form the kernel implements, against torch autograd of `layer` in float64 (both branches); and its
    documented value at an all-zero vector, where autograd has NaN."""
    rs = np.random.RandomState(5)
    fa = torch.from_numpy(rs.standard_normal((2, 64, 3, 2))).clamp_min(0).requires_grad_(True)
    fb = torch.from_numpy(rs.standard_normal((2, 64, 3, 2))).clamp_min(0).requires_grad_(True)
    w, g = torch.from_numpy(rs.uniform(0, 1, 64)), torch.tensor([0.7, -1.3], dtype=torch.float64)
    da, db = torch.autograd.grad((R.layer(fa, fb, w) * g).sum(), (fa, fb))
    assert _rel(R.layer_bwd(fa.detach(), fb.detach(), w, g), da) <= 1e-12
    assert _rel(R.layer_bwd(fb.detach(), fa.detach(), w, g), db) <= 1e-12
    z = fa.detach().clone()
    z[1, :, 2, 1] = 0
    zl = z.clone().requires_grad_(True)
    auto, = torch.autograd.grad((R.layer(zl, fb.detach(), w) * g).sum(), zl)
    assert torch.isnan(auto[1, :, 2, 1]).all(), "torch autograd: 0/0 in the backward of sqrt"
    mine = R.layer_bwd(z, fb.detach(), w, g)
    ub, _ = R.normalize(fb.detach())
    want = (1.0 / R.EPS) * 2.0 * w * (0.0 - ub[1, :, 2, 1]) * g[1] / 6
    assert torch.isfinite(mine).all() and torch.allclose(mine[1, :, 2, 1], want, rtol=1e-12, atol=0)


def test_relu_maxpool2_restatement_is_torch_autograd_and_routes_ties_to_the_first():
    x = torch.tensor([[2., 2., -1., 0., 5.], [2., 1., -3., -2., 5.], [7., 7., 7., 7., 5.]]).view(1, 1, 3, 5).double()
    dy = torch.tensor([[10., 20.]]).view(1, 1, 1, 2).double()
    leaf = x.clone().requires_grad_(True)
    pooled, relu = R.relu_maxpool2(leaf)
    auto, = torch.autograd.grad((pooled * dy).sum(), leaf)
    mine = R.relu_maxpool2_bwd(x, dy)
    assert torch.equal(mine, auto)
    assert mine[0, 0].tolist() == [[10., 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]], "tie -> first; all <= 0 -> nothing; odd row / column -> 0"
    assert torch.equal(R.relu_maxpool2_bwd(relu.detach(), dy), mine), "the post-ReLU map gives the same routing"


@pytest.mark.parametrize("use_dropout", [True, False])
def test_state_dict_key_layout(use_dropout):
    from dsml_thesis_amd import synth
    from dsml_thesis_amd.lpips import LPIPS
    sd = synth.lpips_state_dict(3, use_dropout=use_dropout)
    idx = 1 if use_dropout else 0
    want = ["scaling_layer.shift", "scaling_layer.scale"]
    for k, convs in ((1, (0, 2)), (2, (5, 7)), (3, (10, 12, 14)), (4, (17, 19, 21)), (5, (24, 26, 28))):
        want += [f"net.slice{k}.{i}.{s}" for i in convs for s in ("weight", "bias")]
    want += [f"lin{k}.model.{idx}.weight" for k in range(5)]
    assert list(sd) == want
    assert sd["net.slice1.0.weight"].shape == (64, 3, 3, 3) and sd["net.slice4.17.weight"].shape == (512, 256, 3, 3)
    assert [tuple(sd[f"lin{k}.model.{idx}.weight"].shape) for k in range(5)] == [(1, c, 1, 1) for c in (64, 128, 256, 512, 512)]
    assert sd["scaling_layer.shift"].shape == (1, 3, 1, 1) and sum(v.numel() for v in sd.values()) == 14714688 + 1472 + 6
    assert all(v.dtype == torch.float32 for v in sd.values())
    assert all((sd[f"lin{k}.model.{idx}.weight"] >= 0).all() for k in range(5))
    again = synth.lpips_state_dict(3, use_dropout=use_dropout)
    assert all(torch.equal(sd[k], again[k]) for k in sd) and not torch.equal(sd["net.slice1.0.weight"], synth.lpips_state_dict(4)["net.slice1.0.weight"])
    m = LPIPS(use_dropout=use_dropout)
    assert list(m.state_dict()) == want, "the module's own keys are the reference's"
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert not m.training and not m.train().training, "eval-only"
    assert not any(p.requires_grad for p in m.parameters())


def test_target_map_resolves_both_reference_names():
    from dsml_thesis_amd import util
    from dsml_thesis_amd.lpips import LPIPS
    for name in ("taming.modules.losses.lpips.LPIPS", "ldm.modules.losses.lpips.LPIPS"):
        assert util.get_obj_from_str(name) is LPIPS
    m = util.instantiate_from_config(dict(target="taming.modules.losses.lpips.LPIPS", params=dict(use_dropout=False)))
    assert isinstance(m, LPIPS) and "lin0.model.0.weight" in m.state_dict()


def test_forward_without_weights_is_refused_with_a_message(tmp_path):
    from dsml_thesis_amd import synth
    from dsml_thesis_amd.lpips import LPIPS
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(RuntimeError, match="no weights loaded"):
        LPIPS()(x, x)
    with pytest.raises(RuntimeError, match="no weights loaded"):
        LPIPS().value_and_grad(x, x)
    sd = synth.lpips_state_dict(1)
    lin_only = {k: v for k, v in sd.items() if k.startswith("lin")}
    m = LPIPS()
    m.load_state_dict(lin_only, strict=False)
    with pytest.raises(RuntimeError, match="VGG16 convolutions"):
        m(x, x)
    torch.save({k: v for k, v in sd.items() if k.startswith("net.slice1")}, tmp_path / "part.pth")
    with pytest.raises(KeyError, match="lacks"):
        LPIPS(vgg_ckpt=str(tmp_path / "part.pth"))
    m.load_state_dict(sd)
    with pytest.raises(ValueError, match="float32 CUDA image batch"):
        m(x, x)                                             # weights present: now the CPU images are what is refused


@pytest.mark.parametrize("cls", ["VQLPIPSWithDiscriminator", "LPIPSWithDiscriminator"])
def test_loss_classes_still_refuse_a_missing_perceptual_network(cls):
    from dsml_thesis_amd import losses
    with pytest.raises(NotImplementedError, match="cannot be obtained offline") as e:
        getattr(losses, cls)(disc_start=0, perceptual_weight=1.0)
    assert "dsml_thesis_amd.lpips.LPIPS" in str(e.value), "the advice names the class that now exists"
    assert getattr(losses, cls)(disc_start=0, perceptual_weight=0.0).perceptual_loss is None
