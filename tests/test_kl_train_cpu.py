"""CPU: the KL first-stage training surface that needs no GPU -- the factory targets, the constructor refusals, the loss's
host arithmetic against the reference's recorded logs (tests/golden/g24_kl_train.npz), the fixture's shape, and the new
symbols in header, binding and library with their host-side argument checks."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ldmk_gauss_kl_fwd", "ldmk_gauss_kl_bwd", "ldmk_l1_sum_grad"]
LOSS_A = dict(disc_start=0, logvar_init=0.0, kl_weight=1e-6, disc_num_layers=2, disc_weight=0.8, perceptual_weight=1.0)
LOSS_B = dict(LOSS_A, logvar_init=-0.7, kl_weight=0.05)
KL_TARGET = "ldm.modules.losses.contperceptual.LPIPSWithDiscriminator"


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
    assert "kl_train.hip" in SOURCES


def test_kernels_validate_before_launch(lib):
    p = 4096                                         # never dereferenced
    assert lib.ldmk_gauss_kl_fwd(p, None, p, p, 2, 3, 0, p, None) == -1
    assert b"ldmk_gauss_kl_fwd: bad args" in lib.ldmk_last_error()
    assert lib.ldmk_gauss_kl_fwd(p, None, p, p, 2, 3, 4, None, None) == -1            # no scratch
    assert lib.ldmk_gauss_kl_fwd(p, None, None, p, 2, 3, 4, p, None) == -1            # no z
    assert lib.ldmk_gauss_kl_fwd(p, None, p, p, 65536, 3, 4, p, None) == -1
    assert b"above 65535" in lib.ldmk_last_error()
    assert lib.ldmk_gauss_kl_bwd(p, None, None, 1.0, None, 2, 3, 4, None) == -1
    assert b"ldmk_gauss_kl_bwd: bad args" in lib.ldmk_last_error()
    assert lib.ldmk_gauss_kl_bwd(p, p, p, 1.0, p, 2, 0, 4, None) == -1
    assert lib.ldmk_l1_sum_grad(p, p, p, 0, 1.0, p, p, None) == -1
    assert lib.ldmk_l1_sum_grad(p, p, p, 8, 1.0, None, p, None) == -1
    assert b"ldmk_l1_sum_grad: bad args" in lib.ldmk_last_error()


def test_wrappers_refuse_on_the_host():
    from dsml_thesis_amd import lib as L, train_ops as T
    with pytest.raises(L.LdmkError, match="contiguous float32 CUDA tensor"):
        T.gauss_kl_fwd(torch.zeros(1, 6, 2, 2))
    with pytest.raises(L.LdmkError, match="contiguous float32 CUDA tensor"):
        T.l1_sum_grad(torch.zeros(4), torch.zeros(4), 1.0)


def test_factory_targets_resolve():
    from dsml_thesis_amd import losses as Ls
    from dsml_thesis_amd.util import get_obj_from_str, instantiate_from_config
    assert get_obj_from_str(KL_TARGET) is Ls.LPIPSWithDiscriminator
    assert get_obj_from_str("ldm.modules.losses.LPIPSWithDiscriminator") is Ls.LPIPSWithDiscriminator
    loss = instantiate_from_config(dict(target=KL_TARGET, params=dict(disc_start=3, perceptual_weight=0.0, logvar_init=-0.7)))
    assert isinstance(loss, Ls.LPIPSWithDiscriminator) and loss.discriminator_iter_start == 3
    assert isinstance(loss.logvar, torch.nn.Parameter) and loss.logvar.shape == () and loss.logvar.item() == pytest.approx(-0.7)
    assert "logvar" in loss.state_dict() and "discriminator.main.0.weight" in loss.state_dict()


def test_constructor_refusals():
    from dsml_thesis_amd import losses as Ls, synth
    from dsml_thesis_amd.autoencoder import AutoencoderKL
    with pytest.raises(NotImplementedError, match="cannot be obtained offline"):
        Ls.LPIPSWithDiscriminator(disc_start=0)
    for kw in (dict(use_actnorm=True), dict(disc_conditional=True)):
        with pytest.raises(NotImplementedError):
            Ls.LPIPSWithDiscriminator(disc_start=0, perceptual_weight=0.0, **kw)
    with pytest.raises(ValueError):
        Ls.LPIPSWithDiscriminator(disc_start=0, perceptual_weight=0.0, disc_loss="wgan")
    stand_in = torch.nn.Identity()
    assert Ls.LPIPSWithDiscriminator(disc_start=0, perceptual_loss=stand_in).perceptual_loss is stand_in
    loss = Ls.LPIPSWithDiscriminator(disc_start=0, perceptual_weight=0.0)
    x = torch.zeros(1, 3, 8, 8)
    for kw in (dict(cond=x), dict(weights=x)):
        with pytest.raises(NotImplementedError, match="cond .* and weights"):
            loss(x, x, torch.zeros(1), 0, 0, **kw)
    c = synth.KL_TRAIN_SMALL
    m = AutoencoderKL(ddconfig=dict(c["ddconfig"]), embed_dim=c["embed_dim"],
                      lossconfig=dict(target=KL_TARGET, params=dict(disc_start=0, perceptual_weight=0.0, disc_num_layers=2)))
    assert not any(k.startswith("loss.") for k, _ in m.named_parameters()), "the loss stays out of the module tree"
    sd = m.state_dict()
    assert "loss.logvar" in sd and "loss.discriminator.main.0.weight" in sd and "quantize.embedding.weight" not in sd
    opts, scheds = m.configure_optimizers()
    assert len(opts) == 2 and scheds == [] and opts[0].betas == (0.5, 0.9)
    assert isinstance(opts[1], torch.optim.Adam) and opts[1].defaults["betas"] == (0.5, 0.9)
    assert m.get_last_layer() is m.decoder.conv_out.weight
    assert m.get_input(dict(image=torch.zeros(2, 8, 8, 3)), "image").shape == (2, 3, 8, 8)
    # the Identity lossconfig of every LatentDiffusion config: no loss entries, and training_step says why it cannot run
    from dsml_thesis_amd import lib as L
    ident = AutoencoderKL(ddconfig=dict(c["ddconfig"]), embed_dim=c["embed_dim"], lossconfig=dict(target="torch.nn.Identity"))
    assert list(ident.state_dict()) == [k for k, _ in ident.named_parameters()]
    with pytest.raises(L.LdmkError, match="no training loss"):
        ident.training_step(dict(image=torch.zeros(2, 32, 32, 3)), 0, 0)
    # a dropout or wide-boundary config is refused by the trainer before any launch (needs packed weights: GPU only), so
    # here only the refusal that precedes packing
    from dsml_thesis_amd.train_first_stage import FirstStageTrainer
    drop = AutoencoderKL(ddconfig=dict(c["ddconfig"], dropout=0.1), embed_dim=3, lossconfig=dict(target="torch.nn.Identity"))
    with pytest.raises(NotImplementedError, match="dropout"):
        FirstStageTrainer(drop)


def test_state_dict_nested_in_a_parent_module():
    from dsml_thesis_amd import synth
    from dsml_thesis_amd.autoencoder import AutoencoderKL
    c = synth.KL_TRAIN_SMALL

    def parent(seed):
        torch.manual_seed(seed)
        p = torch.nn.Module()
        p.first_stage_model = AutoencoderKL(ddconfig=dict(c["ddconfig"]), embed_dim=c["embed_dim"],
                                            lossconfig=dict(target=KL_TARGET, params=dict(disc_start=0, perceptual_weight=0.0,
                                                                                          disc_num_layers=2, logvar_init=0.25)))
        return p
    a, b = parent(1), parent(2)
    sd = a.state_dict()
    assert "first_stage_model.loss.logvar" in sd and sd["first_stage_model.loss.logvar"].item() == 0.25
    with torch.no_grad():
        b.first_stage_model.loss.logvar.fill_(-1.0)
    res = b.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for (k, v), w in zip(sd.items(), b.state_dict().values()):
        assert torch.equal(v, w), k
    with pytest.raises(RuntimeError, match="loss.logvar"):
        b.load_state_dict({k: v for k, v in sd.items() if not k.endswith("loss.logvar")}, strict=True)


@pytest.mark.parametrize("tag,loss_kw,shape", [("a", LOSS_A, (2, 32, 32, 3)), ("b", LOSS_B, (2, 32, 48, 3))])
def test_loss_host_arithmetic_against_the_fixture_logs(tag, loss_kw, shape):
    """`LPIPSWithDiscriminator.assemble` fed the fixture's own reconstruction and moments, the perceptual stand-in on the CPU
    and a zero GAN term: nll, kl and rec_loss match the reference's logs, and the total matches the reference's total less
    its recorded GAN term.  Everything here is fp32 sums over <= 9216 elements on both sides: 2e-5 relative, the bound the
    GPU test holds the logs to."""
    from conftest import golden, rnd
    from dsml_thesis_amd import losses as Ls
    from dsml_thesis_amd.distributions import DiagonalGaussianDistribution
    g = golden("g24_kl_train.npz")
    loss = Ls.LPIPSWithDiscriminator(perceptual_loss=Ls.StandInPerceptual(int(g["perceptual_seed"])), **loss_kw)
    # the recipe fills the loss's networks under their `loss.` keys, as loading it into the whole model does
    from dsml_thesis_amd import synth
    shapes = {"loss." + k: tuple(v.shape) for k, v in loss.state_dict().items() if v.dtype.is_floating_point and v.dim() > 0}
    loss.load_state_dict({k[5:]: v for k, v in synth.synth_state_dict(shapes).items()}, strict=False)
    x = torch.tanh(rnd(501, *shape)).permute(0, 3, 1, 2).contiguous()
    xrec = torch.from_numpy(g[f"{tag}_xrec0"])
    kl = DiagonalGaussianDistribution(torch.from_numpy(g[f"{tag}_moments"])).kl()
    with torch.no_grad():
        p_sum = loss.perceptual_loss(x, xrec).sum()
    n, chw = x.shape[0], x[0].numel()
    zero = torch.zeros(())
    total, log = loss.assemble((x - xrec).abs().sum(), p_sum, kl, zero, zero, 1.0, n, chw, split="train")
    want = {k[len(tag) + 5:]: float(g[k]) for k in g.files if k.startswith(f"{tag}_log.")}
    assert set(log) == {"train/total_loss", "train/logvar", "train/kl_loss", "train/nll_loss", "train/rec_loss", "train/d_weight",
                        "train/disc_factor", "train/g_loss"} and set(log) | {"train/disc_loss", "train/logits_real",
                                                                             "train/logits_fake"} == set(want)
    for k in ("train/nll_loss", "train/kl_loss", "train/rec_loss"):
        assert abs(log[k].item() - want[k]) <= 2e-5 * abs(want[k]), (k, log[k].item(), want[k])
    assert log["train/logvar"].item() == want["train/logvar"] == pytest.approx(loss_kw["logvar_init"])
    gan = want["train/d_weight"] * want["train/disc_factor"] * want["train/g_loss"]
    assert abs(total.item() - (want["train/total_loss"] - gan)) <= 2e-5 * abs(want["train/total_loss"])
    assert abs(total.item() - (want["train/nll_loss"] + loss_kw["kl_weight"] * want["train/kl_loss"])) <= 2e-5 * abs(total.item())


@pytest.mark.parametrize("tag", ["a", "b"])
def test_g24_fixture_is_well_formed_and_records_its_conditions(tag):
    """tests/golden/g24_kl_train.npz (tools/make_golden_kl_train.py): arrays and name lists only, under 1 MiB; a's d_weight
    strictly inside the clamp, b's on it; every raw log-variance strictly inside (-30, 20); each recorded draw is
    mean + std * noise bit for bit; the float64 twin has every quantity the fp32 record has."""
    from conftest import golden
    g = golden("g24_kl_train.npz")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g24_kl_train.npz")) < 1 << 20
    assert all(g[k].dtype.kind in "fiuU" for k in g.files), "numbers and strings only"
    keys, shapes = g[f"{tag}_keys"].tolist(), g[f"{tag}_shapes"].tolist()
    assert len(keys) == len(shapes) == len(set(keys)) and "loss.logvar" in keys and "loss.discriminator.main.0.weight" in keys
    assert shapes[keys.index("loss.logvar")] == ""
    names = g[f"{tag}_grad_names"].tolist()
    assert set(names) == {k for k in keys if not k.startswith("loss.")}
    dw = float(g[f"{tag}_log.train/d_weight"]) / 0.8
    assert (0.0 < dw < 1e4) if tag == "a" else dw == 1e4
    mom = torch.from_numpy(g[f"{tag}_moments"])
    e = mom.shape[1] // 2
    assert -30.0 < mom[:, e:].min().item() and mom[:, e:].max().item() < 20.0
    for i in (0, 1):
        z, noise = torch.from_numpy(g[f"{tag}_z{i}"]), torch.from_numpy(g[f"{tag}_noise{i}"])
        assert torch.equal(z, mom[:, :e] + torch.exp(0.5 * mom[:, e:]) * noise)
    assert not torch.equal(torch.from_numpy(g[f"{tag}_noise0"]), torch.from_numpy(g[f"{tag}_noise1"]))
    for suffix in ("", "_f64"):
        assert g[f"{tag}_grad_stats{suffix}"].shape == (len(names), 2)
        assert len([k for k in g.files if k.startswith(f"{tag}_log{suffix}.")]) == 11
        assert len([k for k in g.files if k.startswith(f"{tag}_grad{suffix}.")]) == 10
        assert g[f"{tag}_disc_grad_norms{suffix}"].shape == g[f"{tag}_disc_names"].shape
        assert g[f"{tag}_xrec0{suffix}"].shape == g[f"{tag}_xrec1{suffix}"].shape
    assert g[f"{tag}_xrec0_f64"].dtype == "float64" and g[f"{tag}_grad_f64.quant_conv.weight"].dtype == "float64"
