"""CPU: the first-stage training kernels are declared, bound and exported, and refuse bad arguments on the host before
any launch (no GPU needed: validation precedes the launch, as tests/test_abi.py shows for the other entry points)."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ldmk_vq_loss_bwd", "ldmk_vq_codebook_grad", "ldmk_conv1x1_nchw_bwd", "ldmk_l1_grad"]


@pytest.fixture(scope="module")
def lib():
    from dsml_thesis_amd.build import build_lib
    build_lib(verbose=False)
    from dsml_thesis_amd import lib as L
    return L.load()


def test_new_symbols_in_header_binding_and_library(lib):
    from dsml_thesis_amd import lib as L
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ldmk.h")).read(), flags=re.S)
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, hdr), f"{s} not declared in include/ldmk.h"
        assert s in L.EXPORTED and hasattr(lib, s)
    from dsml_thesis_amd.build import SOURCES
    assert "vq_train.hip" in SOURCES


def test_quantiser_kernels_validate_before_launch(lib):
    p = 4096                                         # never dereferenced
    assert lib.ldmk_vq_loss_bwd(p, p, p, None, p, p, 1, 4, 5, 16, 0.25, 1, 1.0, p, None) == -1
    assert b"embed dim 5 unsupported" in lib.ldmk_last_error()
    assert lib.ldmk_vq_loss_bwd(p, p, p, p, None, p, 1, 4, 3, 16, 0.25, 1, 1.0, p, None) == -1
    assert b"dzq without dz" in lib.ldmk_last_error()
    assert lib.ldmk_vq_loss_bwd(p, p, p, None, p, p, 1, 4, 3, 16, 0.25, 1, 1.0, None, None) == -1      # no scratch
    assert lib.ldmk_vq_loss_bwd(p, p, p, None, p, p, 1, 4, 3, 0, 0.25, 1, 1.0, p, None) == -1         # empty codebook
    assert lib.ldmk_vq_codebook_grad(p, p, p, p, None, 1, 4, 2, 16, 0.25, 1, 1.0, None) == -1
    assert b"embed dim 2 unsupported" in lib.ldmk_last_error()
    assert lib.ldmk_vq_codebook_grad(p, p, None, p, None, 1, 4, 3, 16, 0.25, 1, 1.0, None) == -1       # no idx
    assert lib.ldmk_vq_codebook_grad(p, p, p, p, None, 0, 4, 3, 16, 0.25, 1, 1.0, None) == -1


def test_conv1x1_backward_and_l1_validate_before_launch(lib):
    p = 4096
    assert lib.ldmk_conv1x1_nchw_bwd(p, p, p, p, p, p, 1, 4, 9, 3, 0, p, None) == -1
    assert b"must be in [1, 8]" in lib.ldmk_last_error()
    assert lib.ldmk_conv1x1_nchw_bwd(p, p, p, p, p, p, 1, 4, 3, 0, 0, p, None) == -1
    assert lib.ldmk_conv1x1_nchw_bwd(p, p, p, None, None, None, 1, 4, 3, 3, 0, p, None) == -1
    assert b"no output requested" in lib.ldmk_last_error()
    assert lib.ldmk_conv1x1_nchw_bwd(p, p, None, p, None, None, 1, 4, 3, 3, 0, p, None) == -1
    assert b"dx needs the weight" in lib.ldmk_last_error()
    assert lib.ldmk_conv1x1_nchw_bwd(None, p, p, None, p, None, 1, 4, 3, 3, 0, p, None) == -1
    assert b"dw needs the forward input" in lib.ldmk_last_error()
    assert lib.ldmk_conv1x1_nchw_bwd(p, p, p, None, p, p, 1, 4, 3, 3, 0, None, None) == -1
    assert b"need the scratch" in lib.ldmk_last_error()
    assert lib.ldmk_l1_grad(p, p, p, 0, 0, p, p, None) == -1
    assert lib.ldmk_l1_grad(p, p, p, 8, -1, p, p, None) == -1
    assert lib.ldmk_l1_grad(p, p, None, 8, 0, p, p, None) == -1
    assert b"ldmk_l1_grad: bad args" in lib.ldmk_last_error()


def test_wrappers_refuse_on_the_host():
    """The tensor-level wrappers check layouts before they hand pointers to the library."""
    from dsml_thesis_amd import lib as L, train_ops as T
    dy, wd = torch.zeros(1, 2, 2, 32), torch.zeros(9 * 32, 32)
    with pytest.raises(ValueError, match="pad_lo is 1, or 0 with stride 2"):
        T.conv3x3_dgrad(dy, wd, (4, 4), stride=1, pad_lo=0)
    with pytest.raises(ValueError, match="pad_lo"):
        T.conv3x3_dgrad(dy, wd, (4, 4), stride=2, pad_lo=2)
    z, cb = torch.zeros(1, 3, 2, 2), torch.zeros(8, 3)
    with pytest.raises(L.LdmkError, match="contiguous float32 CUDA tensor"):
        T.vq_loss_bwd(z, cb, torch.zeros(4, dtype=torch.int32))
    with pytest.raises(L.LdmkError, match="contiguous float32 CUDA tensor"):
        T.l1_grad(z, z)
    with pytest.raises(L.LdmkError, match="contiguous float32 CUDA tensor"):
        T.conv1x1_nchw_bwd(z, z, torch.zeros(3, 3))


def test_loss_schedule_and_gan_terms_on_cpu_tensors():
    from dsml_thesis_amd import losses as Ls
    assert Ls.adopt_weight(0.7, 9, threshold=10) == 0.0 and Ls.adopt_weight(0.7, 10, threshold=10) == 0.7
    assert Ls.adopt_weight(0.7, 0, threshold=5, value=0.1) == 0.1
    real, fake = torch.tensor([[2.0, 0.5, -1.0]]), torch.tensor([[-2.0, 0.25, 1.0]])
    assert Ls.hinge_d_loss(real, fake).item() == pytest.approx(0.5 * ((0 + 0.5 + 2.0) / 3 + (0 + 1.25 + 2.0) / 3))
    want = 0.5 * (torch.log1p(torch.exp(-real)).mean() + torch.log1p(torch.exp(fake)).mean())
    assert Ls.vanilla_d_loss(real, fake).item() == pytest.approx(want.item(), rel=1e-6)
    perp, used = Ls.perplexity_from_counts(torch.tensor([4, 4, 0, 0]))
    assert perp.item() == pytest.approx(2.0, rel=1e-6) and used.item() == 2
    d = Ls.NLayerDiscriminator(input_nc=3, ndf=16, n_layers=2)
    assert [k for k in d.state_dict() if k.endswith("weight")] == ["main.0.weight", "main.2.weight", "main.3.weight", "main.5.weight",
                                                                   "main.6.weight", "main.8.weight"]
    assert d(torch.zeros(2, 3, 32, 32)).shape == (2, 1, 6, 6)


def test_constructor_refusals():
    from dsml_thesis_amd import losses as Ls, synth
    from dsml_thesis_amd.autoencoder import VQModel
    from dsml_thesis_amd.util import get_obj_from_str
    with pytest.raises(NotImplementedError, match="cannot be obtained offline"):
        Ls.VQLPIPSWithDiscriminator(disc_start=0)
    for kw in (dict(use_actnorm=True), dict(disc_conditional=True)):
        with pytest.raises(NotImplementedError):
            Ls.VQLPIPSWithDiscriminator(disc_start=0, perceptual_weight=0.0, **kw)
    with pytest.raises(ValueError):
        Ls.VQLPIPSWithDiscriminator(disc_start=0, perceptual_weight=0.0, pixel_loss="l3")
    stand_in = torch.nn.Identity()
    assert Ls.VQLPIPSWithDiscriminator(disc_start=0, perceptual_loss=stand_in).perceptual_loss is stand_in
    c = synth.VQ_TRAIN_SMALL
    base = dict(ddconfig=dict(c["ddconfig"]), n_embed=c["n_embed"], embed_dim=c["embed_dim"],
                lossconfig=dict(target="taming.modules.losses.vqperceptual.VQLPIPSWithDiscriminator",
                                params=dict(disc_start=0, perceptual_weight=0.0)))
    for kw in (dict(batch_resize_range=(32, 64)), dict(remap="x.npy"), dict(colorize_nlabels=8), dict(scheduler_config=dict(target="x"))):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            VQModel(**base, **kw)
    assert get_obj_from_str("ldm.models.autoencoder.VQModel") is VQModel is get_obj_from_str("taming.models.vqgan.VQModel")
    m = VQModel(**base)
    assert not any(k.startswith("loss.") for k, _ in m.named_parameters()) and "loss.discriminator.main.0.weight" in m.state_dict()
    opts, scheds = m.configure_optimizers()
    assert len(opts) == 2 and scheds == [] and isinstance(opts[1], torch.optim.Adam) and opts[1].defaults["betas"] == (0.5, 0.9)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_g21_fixture_is_well_formed_and_records_its_two_conditions(tag):
    """tests/golden/g21_vq_train.npz (tools/make_golden_vq_train.py): arrays and name lists only; the quantiser gap is at least
    1e-4 (about 100 x the fp32 rounding of distances of order 1), and codes with 0, 1 and more than 1 hits all occur."""
    from conftest import golden
    g = golden("g21_vq_train.npz")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g21_vq_train.npz")) < 1 << 20
    assert all(g[k].dtype.kind in "fiuU" for k in g.files), "numbers and strings only"
    hist, idx = g[f"{tag}_hist"], g[f"{tag}_idx"]
    assert float(g[f"{tag}_gap"]) >= 1e-4
    assert (hist == 0).any() and (hist == 1).any() and (hist > 1).any()
    assert hist.sum() == idx.size and (torch.bincount(torch.from_numpy(idx).long(), minlength=hist.size).numpy() == hist).all()
    keys, shapes = g[f"{tag}_keys"].tolist(), g[f"{tag}_shapes"].tolist()
    assert len(keys) == len(shapes) == len(set(keys)) and "loss.discriminator.main.0.weight" in keys
    names = g[f"{tag}_grad_names"].tolist()
    assert set(names) == {k for k in keys if not k.startswith("loss.")} and g[f"{tag}_grad_stats"].shape == (len(names), 2)
    assert len([k for k in g.files if k.startswith(f"{tag}_log.")]) == 13 and len([k for k in g.files if k.startswith(f"{tag}_grad.")]) == 10
    assert g[f"{tag}_disc_grad_norms"].shape == g[f"{tag}_disc_names"].shape and int(g["perceptual_seed"]) >= 0
    if tag == "a":                    # what the issue measured with the recipe weights
        assert abs(float(g["a_log.train/quant_loss"]) - 0.148646) < 1e-6 and ((hist == 0).sum(), (hist == 1).sum(), hist.max()) == (20, 7, 37)


def test_vqmodel_state_dict_nested_in_a_parent_module():
    """A VQModel that is a child module (say `first_stage_model`) carries its loss entries under the parent's prefix, and the
    parent's load restores them."""
    from dsml_thesis_amd import synth
    from dsml_thesis_amd.autoencoder import VQModel
    c = synth.VQ_TRAIN_SMALL

    def parent(seed):
        torch.manual_seed(seed)
        p = torch.nn.Module()
        p.first_stage_model = VQModel(ddconfig=dict(c["ddconfig"]), n_embed=c["n_embed"], embed_dim=c["embed_dim"],
                                      lossconfig=dict(target="ldm.modules.losses.vqperceptual.VQLPIPSWithDiscriminator",
                                                      params=dict(disc_start=0, perceptual_weight=0.0, disc_num_layers=2, disc_ndf=16)))
        return p
    a, b = parent(1), parent(2)
    sd = a.state_dict()
    assert all(k.startswith("first_stage_model.") for k in sd) and "first_stage_model.loss.discriminator.main.0.weight" in sd
    assert [k[len("first_stage_model."):] for k in sd] == list(a.first_stage_model.state_dict())
    assert not torch.equal(sd["first_stage_model.loss.discriminator.main.0.weight"], b.state_dict()["first_stage_model.loss.discriminator.main.0.weight"])
    res = b.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for (k, v), w in zip(sd.items(), b.state_dict().values()):
        assert torch.equal(v, w), k
    kept = a.first_stage_model.state_dict(keep_vars=True)
    assert kept["loss.discriminator.main.0.weight"] is a.first_stage_model.loss.discriminator.main[0].weight
    assert kept["encoder.conv_in.weight"] is a.first_stage_model.encoder.conv_in.weight
    with pytest.raises(RuntimeError, match="loss.discriminator.main.0.weight"):
        b.load_state_dict({k: v for k, v in sd.items() if ".loss." not in k}, strict=True)
    with pytest.raises(RuntimeError, match="loss.nope"):
        b.load_state_dict(dict(sd, **{"first_stage_model.loss.nope": torch.zeros(1)}), strict=True)


def test_trainer_refuses_dropout():
    from dsml_thesis_amd import synth
    from dsml_thesis_amd.autoencoder import VQModelInterface
    from dsml_thesis_amd.train_first_stage import FirstStageTrainer
    c = synth.VQ_TRAIN_SMALL
    vq = VQModelInterface(embed_dim=c["embed_dim"], n_embed=c["n_embed"], ddconfig=dict(c["ddconfig"], dropout=0.1),
                          lossconfig=dict(target="torch.nn.Identity"))
    with pytest.raises(NotImplementedError, match="dropout"):
        FirstStageTrainer(vq)
