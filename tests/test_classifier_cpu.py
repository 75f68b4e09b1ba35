"""CPU: the host side of the noisy-latent classifier -- EncoderUNetModel's parameter tree against the reference's
(tests/golden/g26_classifier.npz, tools/make_golden_classifier.py), the config `load_classifier` derives, what is refused, top-k, and
ClassifierGuidance's formula on a stub classifier.  Nothing here launches a kernel."""
import types

import pytest
import torch
import torch.nn as nn

from conftest import golden
from oracle import weights as W

SMALL = dict(W.FR_UNET, model_channels=64, channel_mult=[1, 2], num_res_blocks=1, attention_resolutions=[2, 1])   # g9's TRAIN_UNET
CASES = dict(adaptive=dict(pool="adaptive"), attention=dict(pool="attention"), spatial=dict(pool="spatial"),
             spatial_v2=dict(pool="spatial_v2"), attention_new=dict(pool="attention", use_new_attention_order=True))


def _encoder(**over):
    from dsml_thesis_amd.encoder_unet import EncoderUNetModel
    return EncoderUNetModel(**dict(SMALL, image_size=16, in_channels=3, out_channels=8, **over))


class _StubDiffusion(nn.Module):
    """What NoisyLatentImageClassifier reads of a diffusion model, without a first stage or a GPU."""

    def __init__(self, cond_stage_key="class_label", **extra):
        super().__init__()
        from dsml_thesis_amd.unet import UNetModel
        self.model = types.SimpleNamespace(diffusion_model=UNetModel(**dict(SMALL, image_size=16)))
        self.num_timesteps, self.log_every_t, self.first_stage_key = 1000, 200, "image"
        if cond_stage_key is not None:
            self.cond_stage_key = cond_stage_key
        for k, v in extra.items():
            setattr(self, k, v)


@pytest.mark.parametrize("case", list(CASES))
def test_state_dict_keys_and_shapes_are_the_references(case):
    g = golden("g26_classifier.npz")
    m = _encoder(**CASES[case])                     # the FR UNet's extra kwargs (use_spatial_transformer, ...) are swallowed
    ref = {str(k): tuple(int(s) for s in str(sh).split(",")) for k, sh in zip(g[f"{case}_names"], g[f"{case}_shapes"])}
    mine = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert list(mine) == list(ref), (sorted(set(mine) ^ set(ref)))
    assert mine == ref
    assert m._feature_size == 448 and sum(m.feature_widths) == 448
    assert not any(k.startswith("output_blocks") or "transformer_blocks" in k for k in mine)


def test_zero_module_sites_and_pool_validation():
    m = _encoder(pool="adaptive")
    sd = m.state_dict()
    assert float(sd["out.3.weight"].abs().max()) == 0 and float(sd["out.3.bias"].abs().max()) == 0
    assert float(sd["middle_block.1.proj_out.weight"].abs().max()) == 0 and float(sd["out.0.weight"].min()) == 1
    assert float(_encoder(pool="attention").state_dict()["out.2.c_proj.weight"].abs().max()) > 0
    with pytest.raises(NotImplementedError, match="Unexpected max pooling"):
        _encoder(pool="max")
    with pytest.raises(AssertionError):
        _encoder(pool="attention", num_head_channels=-1, num_heads=2)
    with pytest.raises(NotImplementedError, match="fp32 only"):
        _encoder(use_fp16=True)
    with pytest.raises(NotImplementedError, match="fp32 only"):
        _encoder().convert_to_fp16()


def test_load_classifier_derives_the_config_like_the_reference():
    from dsml_thesis_amd.classifier import NoisyLatentImageClassifier, classifier_config, unet_params_of
    from dsml_thesis_amd.encoder_unet import EncoderUNetModel
    dm = _StubDiffusion()
    params = unet_params_of(dm.model.diffusion_model)
    for k, v in dict(SMALL, image_size=16).items():
        assert params[k] == v, k
    cfg = classifier_config(dict(SMALL, image_size=16, out_channels=4), 8, "spatial")
    assert cfg["in_channels"] == 4 and cfg["out_channels"] == 8 and cfg["pool"] == "spatial" and cfg["context_dim"] == 512
    assert "pool" not in classifier_config(dict(SMALL), 8, "spatial", label_key="segmentation")
    c = NoisyLatentImageClassifier(num_classes=8, pool="spatial_v2", label_key="ignored", diffusion_model=dm)
    assert isinstance(c.model, EncoderUNetModel) and c.model.pool == "spatial_v2"
    assert c.label_key == "class_label"                              # the diffusion model's cond_stage_key wins
    assert c.model.in_channels == 3 and c.model.out_channels == 8 and c.model_config["use_spatial_transformer"] is True
    assert all(k.startswith("model.") for k in c.state_dict())      # the frozen diffusion model is not in the state dict
    assert list(c.noisy_acc) == [0, 200, 400, 600, 800] and c.log_time_interval == 100
    assert NoisyLatentImageClassifier(num_classes=8, label_key="class_label", diffusion_model=_StubDiffusion(None)).label_key == "class_label"


def test_what_is_not_built_raises():
    from dsml_thesis_amd.classifier import NoisyLatentImageClassifier
    with pytest.raises(NotImplementedError, match="segmentation"):
        NoisyLatentImageClassifier(num_classes=8, diffusion_model=_StubDiffusion("segmentation"))
    with pytest.raises(NotImplementedError, match="caption"):
        NoisyLatentImageClassifier(num_classes=8, diffusion_model=_StubDiffusion("caption"))
    with pytest.raises(NotImplementedError, match="Unexpected"):
        NoisyLatentImageClassifier(num_classes=8, pool="max", diffusion_model=_StubDiffusion())
    with pytest.raises(AssertionError, match="label_key"):
        NoisyLatentImageClassifier(num_classes=8, diffusion_model=_StubDiffusion(None))
    c = NoisyLatentImageClassifier(num_classes=8, diffusion_model=_StubDiffusion(use_continuous_noise=True))
    with pytest.raises(NotImplementedError, match="use_continuous_noise"):
        c.get_x_noisy(torch.zeros(1, 3, 16, 16), torch.zeros(1, dtype=torch.int64))
    with pytest.raises(NotImplementedError, match="log_images"):
        c.log_images({})
    with pytest.raises(FileNotFoundError):
        NoisyLatentImageClassifier(diffusion_path="/nonexistent/logs", num_classes=8)


def test_compute_top_k_on_a_hand_case():
    from dsml_thesis_amd.classifier import NoisyLatentImageClassifier
    c = NoisyLatentImageClassifier(num_classes=4, diffusion_model=_StubDiffusion())
    logits = torch.tensor([[0.1, 0.9, 0.3, 0.2], [0.8, 0.1, 0.5, 0.7], [0.0, 0.1, 0.2, 0.3]])
    labels = torch.tensor([1, 3, 0])
    assert c.compute_top_k(logits, labels, 1) == pytest.approx(1 / 3)
    assert c.compute_top_k(logits, labels, 2) == pytest.approx(2 / 3)
    assert c.compute_top_k(logits, labels, 4) == 1.0
    assert c.compute_top_k(logits, labels, 2, reduction="none").tolist() == [1.0, 1.0, 0.0]


def test_get_input_and_conditioning():
    from dsml_thesis_amd.classifier import NoisyLatentImageClassifier
    c = NoisyLatentImageClassifier(num_classes=8, diffusion_model=_StubDiffusion())
    batch = dict(image=torch.arange(2 * 4 * 5 * 3, dtype=torch.float64).view(2, 4, 5, 3), class_label=torch.tensor([1, 7]))
    x = c.get_input(batch, "image")
    assert x.shape == (2, 3, 4, 5) and x.dtype == torch.float32 and x.is_contiguous() and float(x[1, 2, 3, 4]) == float(batch["image"][1, 3, 4, 2])
    assert c.get_input(dict(m=torch.zeros(2, 4, 5)), "m").shape == (2, 1, 4, 5)
    assert c.get_conditioning(batch).tolist() == [1, 7]


def test_classifier_guidance_formula_on_a_stub():
    from dsml_thesis_amd.classifier import ClassifierGuidance
    gen = torch.Generator().manual_seed(0)
    e_t, x, grad = (torch.randn(3, 3, 4, 4, generator=gen) for _ in range(3))
    t = torch.tensor([17, 803, 17])
    table = torch.linspace(0.1, 0.99, 1000)
    seen = {}

    class Stub:
        def log_prob_grad(self, x_, t_, y_):
            seen.update(x=x_, t=t_, y=y_)
            return grad

    model = types.SimpleNamespace(sqrt_one_minus_alphas_cumprod=table)
    cg = ClassifierGuidance(Stub(), scale=2.5)
    with pytest.raises(ValueError, match="corrector_kwargs"):
        cg.modify_score(model, e_t, x, t, None)                     # no guessing of the labels behind c
    out = cg.modify_score(model, e_t, x, t, None, y=torch.tensor([1, 7, 1]))
    want = e_t - table[t].view(3, 1, 1, 1) * 2.5 * grad
    assert torch.equal(out, want)
    assert seen["x"] is x and seen["y"].tolist() == [1, 7, 1] and seen["t"].tolist() == [17, 803, 17]
    out = ClassifierGuidance(Stub(), scale=1.0, y=5).modify_score(model, e_t, x, t, None)
    assert seen["y"].tolist() == [5, 5, 5] and torch.equal(out, e_t - table[t].view(3, 1, 1, 1) * 1.0 * grad)


def test_reference_targets_resolve_to_the_native_classes():
    from dsml_thesis_amd.util import get_obj_from_str
    from dsml_thesis_amd.classifier import NoisyLatentImageClassifier
    from dsml_thesis_amd.encoder_unet import EncoderUNetModel
    assert get_obj_from_str("ldm.modules.diffusionmodules.openaimodel.EncoderUNetModel") is EncoderUNetModel
    assert get_obj_from_str("ldm.models.diffusion.classifier.NoisyLatentImageClassifier") is NoisyLatentImageClassifier


def test_init_from_ckpt_with_ignore_keys_and_only_model(tmp_path):
    from dsml_thesis_amd.classifier import NoisyLatentImageClassifier
    a = NoisyLatentImageClassifier(num_classes=8, diffusion_model=_StubDiffusion())
    sd = a.state_dict()
    path = str(tmp_path / "clf.ckpt")
    torch.save({"state_dict": dict(sd, **{"diffusion_model.betas": torch.zeros(3)})}, path)       # a reference checkpoint also holds the frozen model
    b = NoisyLatentImageClassifier(num_classes=8, diffusion_model=_StubDiffusion(), ckpt_path=path)
    assert all(torch.equal(v, sd[k]) for k, v in b.state_dict().items())
    c = NoisyLatentImageClassifier(num_classes=8, diffusion_model=_StubDiffusion())
    before = c.state_dict()["model.out.2.c_proj.weight"].clone()
    missing, unexpected = c.init_from_ckpt(path, ignore_keys=["model.out.", "diffusion_model."])
    assert unexpected == [] and missing and all(k.startswith("model.out.") for k in missing)
    assert torch.equal(c.state_dict()["model.out.2.c_proj.weight"], before)
    assert torch.equal(c.state_dict()["model.time_embed.0.weight"], sd["model.time_embed.0.weight"])
    torch.save({k[len("model."):]: v for k, v in sd.items()}, path)
    d = NoisyLatentImageClassifier(num_classes=8, diffusion_model=_StubDiffusion())
    d.init_from_ckpt(path, only_model=True)
    assert all(torch.equal(v, sd[k]) for k, v in d.state_dict().items())
