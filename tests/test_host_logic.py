"""CPU: host-side logic of the product package (no kernels run): schedules against the reference's golden
tables, the config factory mapping, state-dict key compatibility, sharding arithmetic, loud failure without a GPU."""
import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden
from oracle import weights as W


def test_schedule_tables_match_reference_goldens():
    from dsml_thesis_amd import schedule as S
    g = golden("g1_schedules.npz")
    bufs = S.schedule_buffers(S.make_beta_schedule("linear", 1000, linear_start=0.0015, linear_end=0.0205))
    for k in ("betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_recip_alphas_cumprod",
              "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1", "posterior_mean_coef2",
              "posterior_log_variance_clipped", "sqrt_one_minus_alphas_cumprod"):
        assert np.array_equal(bufs[k].numpy(), g[k]), k
    for S_ in (50, 200):
        ts = S.make_ddim_timesteps("uniform", S_, 1000)
        assert np.array_equal(ts, g[f"S{S_}_timesteps"])
        for eta in (0.0, 1.0):
            tab = S.ddim_step_table(bufs["alphas_cumprod"], ts, eta)
            for j, name in enumerate(("a_t", "a_prev", "sigma_t", "sqrt_one_minus_at")):
                assert np.array_equal(tab[:, j], g[f"S{S_}_eta{int(eta)}_{name}"]), (S_, eta, name)
    with pytest.raises(IndexError):      # the reference fails the same way when S does not divide 1000 (util.py:49-57)
        S.make_ddim_sampling_parameters(bufs["alphas_cumprod"], S.make_ddim_timesteps("uniform", 3, 1000), 0.0)


def test_config_factory_maps_reference_targets():
    from dsml_thesis_amd.util import get_obj_from_str, instantiate_from_config
    from dsml_thesis_amd.unet import UNetModel
    from dsml_thesis_amd.ddpm import LatentDiffusion, LatentDiffusion2Cond
    assert get_obj_from_str("ldm.modules.diffusionmodules.openaimodel.UNetModel") is UNetModel
    assert get_obj_from_str("ldm.models.diffusion.ddpm.LatentDiffusion") is LatentDiffusion
    assert get_obj_from_str("ldm.models.diffusion.ddpm2cond.LatentDiffusion") is LatentDiffusion2Cond
    m = instantiate_from_config({"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel",
                                 "params": dict(W.FR_UNET, model_channels=32, channel_mult=[1, 2])})
    assert isinstance(m, UNetModel)
    with pytest.raises(KeyError):
        instantiate_from_config({"params": {}})


def test_state_dict_keys_equal_reference_enumeration():
    from helpers import fr_config, tf_config
    from dsml_thesis_amd.ddpm import LatentDiffusion, LatentDiffusion2Cond
    m = LatentDiffusion(**fr_config())
    sd = m.state_dict()
    unet_keys = {"model.diffusion_model." + k: tuple(s) for k, s in W.unet_param_shapes(W.FR_UNET).items()}
    vq_keys = {"first_stage_model." + k: tuple(s) for k, s in W.vqmodel_param_shapes(W.VQ_F4).items()}
    for k, shp in {**unet_keys, **vq_keys}.items():
        assert tuple(sd[k].shape) == shp, k
    # LitEma shadow names: parameter name with the dots removed (ema.py:16-21)
    assert "model_ema.diffusion_modelout2weight" in sd and "model_ema.decay" in sd and "model_ema.num_updates" in sd
    assert sum(1 for k in sd if k.startswith("model_ema.")) == len(unet_keys) + 2
    for k in ("betas", "alphas_cumprod", "posterior_mean_coef1", "cond_stage_model.embedding.weight",
              "cond_stage_model.uncond_embedding.weight"):
        assert k in sd
    m2 = LatentDiffusion2Cond(**tf_config())
    sd2 = m2.state_dict()
    assert sd2["model.diffusion_model.input_blocks.0.0.weight"].shape == (160, 9, 3, 3)
    assert sd2["cond_stage_model_1.embedding.weight"].shape == (9, 256)
    assert sd2["cond_stage_model_2.attentionNet.0.weight"].shape == (17, 17)
    # zero-initialised tensors of a fresh model are the reference's zero_module sites
    z = [k for k, v in m.model.diffusion_model.state_dict().items() if v.dim() > 1 and float(v.abs().max()) == 0.0]
    assert len(z) == 34 and all((".out_layers.3." in k) or (".proj_out." in k) or k.startswith("out.2.") for k in z)


def test_unsupported_options_fail_loudly():
    from dsml_thesis_amd.unet import UNetModel
    from dsml_thesis_amd.autoencoder import VQModelInterface
    for bad in (dict(dims=3), dict(n_embed=8), dict(use_fp16=True),
                dict(num_head_channels=48)):       # (160 channels do not split into whole heads of 48)
        with pytest.raises(NotImplementedError):
            UNetModel(**dict(W.FR_UNET, **bad))
    with pytest.raises(AssertionError):                      # openaimodel.py:474-475: context_dim needs the spatial transformer
        UNetModel(**dict(W.FR_UNET, use_spatial_transformer=False))
    # the unconditional variant (AttentionBlock instead of SpatialTransformer) is built: the reference's key set
    u = UNetModel(**W.UNCOND_UNET)
    assert set(u.state_dict().keys()) == set(W.unet_param_shapes(W.UNCOND_UNET).keys())
    assert u.state_dict()["middle_block.1.qkv.weight"].shape == (1920, 640, 1)
    # head widths other than 32 construct since round 5 (legacy: heads = ch // num_head_channels, width = ch // heads,
    # openaimodel.py:545-549) -- the attention then runs as batched GEMMs instead of the flash kernels
    u64 = UNetModel(**dict(W.FR_UNET, num_head_channels=64))
    assert not u64._heads32 and u64.input_blocks[1].layers[1].heads == 2 and u64.input_blocks[1].layers[1].d_head == 80
    assert UNetModel(**W.FR_UNET)._heads32
    # resblock_updown constructs since round 5: ResBlocks (same keys as a plain block) where Downsample / Upsample would stand
    ud = UNetModel(**W.UPDOWN_UNET)
    assert set(ud.state_dict().keys()) == set(W.unet_param_shapes(W.UPDOWN_UNET).keys())
    assert [m.updown for _, m in ud._walk() if m.kind == "res" and m.updown] == ["down", "down", "up", "up"]
    assert not any(m.kind in ("down", "up") for _, m in ud._walk())
    assert ud.convert_to_fp32() is None                      # (openaimodel.py:702-708: a no-op on an fp32 model)
    with pytest.raises(NotImplementedError):
        ud.convert_to_fp16()
    with pytest.raises(NotImplementedError):
        VQModelInterface(embed_dim=3, n_embed=16, ddconfig=dict(W.VQ_F4["ddconfig"], attn_type="linear"))


def test_no_cpu_fallback():
    from dsml_thesis_amd import lib as L
    from dsml_thesis_amd.unet import UNetModel
    m = UNetModel(**dict(W.FR_UNET, model_channels=32, channel_mult=[1], attention_resolutions=[1]))
    with pytest.raises(L.LdmkError, match="CUDA|GPU"):
        m(torch.zeros(1, 3, 8, 8), torch.zeros(1, dtype=torch.long), context=torch.zeros(1, 1, 512))


def test_shard_ranges_and_item_noise():
    from dsml_thesis_amd.parallel import shard_range, item_noise, batch_noise
    for n in (1, 7, 16, 128, 130):
        for g in (1, 2, 3, 4, 8):
            spans = [shard_range(n, g, r) for r in range(g)]
            covered = [i for lo, hi in spans for i in range(lo, hi)]
            assert covered == list(range(n)), (n, g, spans)
            assert max(hi - lo for lo, hi in spans) == -(-n // g)
    assert shard_range(128, 8, 3) == (48, 64)
    full = batch_noise(11, 0, 6, (3, 4, 4))
    parts = torch.cat([batch_noise(11, lo, hi, (3, 4, 4)) for lo, hi in (shard_range(6, 4, r) for r in range(4))])
    assert torch.equal(full, parts)
    assert not torch.equal(item_noise(11, 0, (3, 4, 4)), item_noise(12, 0, (3, 4, 4)))


def test_tuned_plan_table_is_legal_and_nearest():
    """dsml_thesis_amd/igemm_plans.json (tools/autotune.py): every entry must be launchable for its bucket, and the
    lookup must be a pure function of the shape (same answer on every rank)."""
    from dsml_thesis_amd import engine, lib as L
    table = engine.plan_table()
    assert table, "tuned plan table missing"
    wk = {1: 1, 2: 2, 3: 4, 4: 2, 5: 1, 6: 2}
    for key, rows in table.items():
        n, k, mode, tf, epi, nb = (int(v) for v in key.split(",")[:6])      # optional suffixes: ",bt", ",s<stride>u<ups>"
        assert [r[0] for r in rows] == sorted(r[0] for r in rows)
        row_tiles = {7: (1, 5), 8: (2, 5), 9: (1, 4), 10: (2, 4), 11: (1, 2), 12: (1, 1)}
        slab_tiles = {13: (2, 1, 4), 14: (2, 2, 4), 15: (1, 1, 4), 16: (1, 2, 4), 17: (1, 1, 8), 18: (1, 1, 16), 19: (2, 1, 8), 20: (1, 2, 8)}
        for m, cfg, sk in rows:
            assert 1 <= cfg <= 20 and sk in (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64)
            if cfg > 12:           # slab GEMM (small row counts): whole column tiles, every wave owns >= 1 eight-deep K block;
                tm, tn, nw = slab_tiles[cfg]          # GEGLU splits K only when the consumer reduces (raw slabs)
                assert m <= 4096 and n % (32 * tn) == 0 and nw * sk <= k // 8 and (epi != 1 or tn % 2 == 0) and "bt" not in key
                assert mode == 0 or ",s" not in key   # stride-1 3x3 convolutions only
                continue
            if cfg > 6:            # wave-autonomous row GEMM: rows mode only, K never split, whole column tiles
                tm, tn = row_tiles[cfg]
                assert mode == 0 and sk == 1 and n % (32 * tn) == 0 and (epi != 1 or tn % 2 == 0) and "bt" not in key
                continue
            if epi == 1:
                assert cfg in (1, 2, 3) and sk == 1
            if sk > 1:
                assert (-(-(k // 32) // wk[cfg])) // sk >= 1      # every slab owns at least one K slice
    a = L.IgemmArgs()
    a.N, a.K, a.a_mode, a.a_tf, a.epi, a.batch = 320, 2880, 1, 0, 0, 1
    assert engine.tuned_plan(a, 65536) == engine.tuned_plan(a, 65536)
    near = engine.tuned_plan(a, 57344)            # batch 14: between the tuned 49152 and 65536 buckets
    assert near in (engine.tuned_plan(a, 49152), engine.tuned_plan(a, 65536))
    # far from anything tuned: no plan (the C++ heuristic decides) -- unless the JOB is far from every tuned batch
    # (engine.far_from_tuned: Program.far_plans), when the nearest tuned plan is carried whatever the distance (round 5; rounds
    # 1-4 always gave up beyond a factor 2, which left whole batch ranges without a split-arithmetic plan)
    assert engine.tuned_plan(a, 7) is None
    assert engine.tuned_plan(a, 7, far=True) == engine.tuned_plan(a, min(r[0] for r in table["320,2880,1,0,0,1"]))
    assert [engine.far_from_tuned(b) for b in (1, 2, 4, 7, 8, 16, 32, 33, 48, 63, 64, 128, 256, 257)] == \
        [True, True, True, True, False, False, False, True, True, True, False, False, False, True]
    a.N = 321
    assert engine.tuned_plan(a, 65536) is None    # a shape nobody tuned: the C++ heuristic decides


def test_one_plan_file_with_a_section_per_arithmetic(monkeypatch, tmp_path):
    """dsml_thesis_amd/igemm_plans.json holds every tuned plan, one section per arithmetic / operand form; the LDMK_*_TABLE
    overrides replace ONE section with a flat file (what the tuning tools write) or with that section of another merged file;
    switching an arithmetic off empties its sections."""
    import json
    from dsml_thesis_amd import engine
    for v in ("LDMK_SPLIT_BF16", "LDMK_F16X2", "LDMK_PS", "LDMK_NO_PLAN_TABLE", *engine._SECTIONS.values()):
        monkeypatch.delenv(v, raising=False)
    engine.reset_tables()
    raw = json.load(open(engine._PLAN_FILE))
    assert set(raw) == set(engine._SECTIONS), set(raw)
    for sec in engine._SECTIONS:
        assert sum(len(v) for v in engine.table(sec).values()) == len(raw[sec]) > 0, sec
    # pre-split plans: only the tiles csrc/igemm_ps.hip implements (23..33), GEGLU on the (value, gate)-pair tiles without split-K
    for sec in ("ps_bf16x3", "ps_f16x2"):
        for key, rows in engine.table(sec).items():
            n, k, mode, tf, epi, nb = (int(v) for v in key.split(",")[:6])
            assert mode in (0, 1) and k % 32 == 0 and n % 32 == 0
            for m, cfg, sk in rows:
                assert 23 <= cfg <= 33 and 1 <= sk <= k // 32 and (epi != 1 or (cfg in (25, 28, 32, 33) and sk == 1)), (key, cfg, sk)
                if mode == 1:      # a 3x3 convolution on the conv-mode tile: F16X2 only, four tile shapes, K split on 32-channel chunks
                    assert sec == "ps_f16x2" and cfg in (23, 24, 26, 27) and k % (9 * 32) == 0 and (k // (9 * 32)) % sk == 0 and tf == 0 and epi == 0
    # nearest row count, whatever the distance
    rest = next(k for k in engine.table("ps_f16x2") if k.split(",")[2] == "0")
    assert engine.ps_plan(rest, 3, h2=True) is None and engine.ps_plan(rest, 3, h2=True, far=True) is not None
    assert engine.ps_plan(rest, 1 << 22, h2=True, far=True) is not None
    assert engine.ps_plan("31,64,0,0,0,1", 4096, h2=True) is None
    flat = tmp_path / "flat.json"
    flat.write_text(json.dumps({"4096,64,64,0,0,0,1": [27, 1]}))
    monkeypatch.setenv("LDMK_PS_H2_TABLE", str(flat))
    engine.reset_tables()
    assert engine.ps_plan("64,64,0,0,0,1", 4096, h2=True) == (27, 1) and len(engine.table("ps_f16x2")) == 1
    assert len(engine.table("f16x2")) > 10            # the other sections still come from the plan file
    merged = tmp_path / "merged.json"
    merged.write_text(json.dumps({"ps_f16x2": {"4096,96,96,0,0,0,1": [23, 2]}, "f32": {}}))
    monkeypatch.setenv("LDMK_PS_H2_TABLE", str(merged))
    engine.reset_tables()
    assert engine.ps_plan("96,96,0,0,0,1", 5000, h2=True) == (23, 2)
    monkeypatch.delenv("LDMK_PS_H2_TABLE")
    monkeypatch.setenv("LDMK_F16X2", "0")
    engine.reset_tables()
    assert engine.table("f16x2") == {} and engine.table("ps_f16x2") == {} and engine.table("ps_bf16x3") and engine.table("bf16x3")
    monkeypatch.delenv("LDMK_F16X2")
    engine.reset_tables()


def test_arithmetic_sites_name_flags_and_denials():
    """engine.ArithSites (CPU tensors here): one flag word per named site, the same word for the same name in every program;
    raised() names exactly the words that are up and clears them; a denied site gets no flag (its launches run in bf16x3)."""
    import torch
    from dsml_thesis_amd.engine import ArithSites, NetBuilder

    class _Pg:
        h2_flag = None
    s = ArithSites("cpu")
    a, b = s.flag("blk.0.attn1"), s.flag("blk.0.ff")
    assert a.data_ptr() == s.flag("blk.0.attn1").data_ptr() != b.data_ptr() and a.numel() == 1
    assert s.raised() == []
    b.fill_(1)
    assert s.raised(clear=False) == ["blk.0.ff"] and s.raised() == ["blk.0.ff"] and s.raised() == []
    s.denied.add("blk.0.ff")
    assert s.flag("blk.0.ff") is None and s.flag("blk.0.attn1") is not None
    nb = NetBuilder.__new__(NetBuilder)
    nb.pg, nb.sites, nb.h2_flag = _Pg(), s, None
    with nb.site("blk.0.attn1") as hf:
        assert hf is nb.h2_flag is nb.pg.h2_flag and hf.data_ptr() == a.data_ptr()
        with nb.site("blk.0.ff") as hf2:
            assert hf2 is None and nb.h2_flag is None and nb.pg.h2_flag is None
        assert nb.h2_flag is hf
    assert nb.h2_flag is None and nb.pg.h2_flag is None
    nb.sites, nb.h2_flag = None, a                # a builder driven by hand keeps the flag its caller set
    with nb.site("anything") as hf:
        assert hf is a and nb.h2_flag is a


def test_x3_plan_table_is_legal(monkeypatch):
    """The bf16x3 section of the plan file (tools/autotune.py --x3): the shapes that run in the fp32-accurate bf16x3 arithmetic.
    Only the tiles that implement it (LDS-tiled 1 / 2 / 4 / 5, warp-specialised 21 / 22), never a b_trans shape, GEGLU on an
    even-TN tile without split-K, every slab at least one 32-deep chunk; LDMK_SPLIT_BF16=0 empties the table."""
    from dsml_thesis_amd import engine
    engine.reset_tables()
    monkeypatch.delenv("LDMK_SPLIT_BF16", raising=False)
    monkeypatch.delenv("LDMK_X3_TABLE", raising=False)
    table = engine.x3_table()
    assert len(table) > 50, "x3 plan table missing"
    for key, rows in table.items():
        n, k, mode, tf, epi, nb = (int(v) for v in key.split(",")[:6])
        assert "bt" not in key and k % 32 == 0 and n % 4 == 0
        for m, cfg, sk in rows:
            assert cfg in (1, 2, 4, 5, 21, 22) and 1 <= sk <= 64 and sk <= k // 32
            if epi == 1:
                assert cfg in (1, 2, 22) and sk == 1
            if cfg in (21, 22):
                assert ",s" not in key or "u0" in key          # no upsampling folded into the gather on those tiles
    engine.reset_tables()
    monkeypatch.setenv("LDMK_SPLIT_BF16", "0")
    assert engine.x3_table() == {} and not engine.split_enabled()
    engine.reset_tables()


def test_product_side_recipe_matches_the_oracle_copy():
    """dsml_thesis_amd/synth.py (benchmarks, tools, smoke) and oracle/weights.py (checker) must describe the same models."""
    from dsml_thesis_amd import synth as S
    from oracle import weights as W
    for name in ("FR_UNET", "TF_UNET", "NS_UNET", "VQ_F4", "VQ_F4_256", "SCHEDULE"):
        assert getattr(S, name) == getattr(W, name), name
    for key, shape in (("input_blocks.1.0.in_layers.2.weight", (8, 4, 3, 3)), ("x.bias", (7,)), ("norm.weight", (5,)),
                       ("embedding.weight", (8, 16)), ("time_embed.0.weight", (6, 3))):
        for seed, gain in ((0, 1.0), (3, 0.25)):
            assert np.array_equal(S.synth_tensor(key, shape, seed, gain), W.synth_tensor(key, shape, seed, gain)), key


def test_gradient_bucket_plan():
    """Bucketed all-reduce overlapped with backward: buckets are disjoint tail slices that cover the flat buffer, each
    is handed over only after every closure owning part of it has run, and a tape out of parameter order is refused."""
    from dsml_thesis_amd.train import plan_buckets
    offs = [900, 700, 650, 400, 100, 0]                      # execution order = reverse forward order
    b = plan_buckets(offs, 1000, 250)
    assert b == {1: (700, 1000), 3: (400, 700), 4: (100, 400), 5: (0, 100)}
    cover = sorted(b.values())
    assert cover[0][0] == 0 and cover[-1][1] == 1000 and all(a[1] == c[0] for a, c in zip(cover, cover[1:]))
    for i, (lo, hi) in b.items():                            # nothing still to run owns an offset inside the bucket
        assert all(o < lo for o in offs[i + 1:])
    assert plan_buckets(offs, 1000, 10 ** 9) == {5: (0, 1000)}          # one bucket = the plain all-reduce
    assert plan_buckets([0], 64, 16) == {0: (0, 64)}
    with pytest.raises(ValueError):
        plan_buckets([500, 800, 0], 1000, 100)


# ---- the shipped YAMLs: the `model` section of each, stored under tests/golden/configs/ ----------------------------
_YAMLS = {
    "fr": "affectnet-128-ldm-vq-f4.yaml",          # face_reenactment/configs/latent-diffusion/
    "fr_clip": "affectnet-128-clip-ldm-vq-f4.yaml",  # face_reenactment/configs/latent-diffusion/
    "tf": "mead-128-ldm-f4.yaml",                  # talking_face/configs/latent-diffusion/
}


def _strip_ckpt(node):
    """Drop every `ckpt_path` (checkpoints are not in the repository) -- the only edit made to a shipped config."""
    if isinstance(node, dict):
        return {k: _strip_ckpt(v) for k, v in node.items() if k != "ckpt_path"}
    if isinstance(node, list):
        return [_strip_ckpt(v) for v in node]
    return node


@pytest.mark.parametrize("which", sorted(_YAMLS))
def test_shipped_yaml_instantiates_and_matches_the_enumerated_layout(which):
    """the YAML `target:` factory is the drop-in boundary.  The three shipped model configs are read with
    yaml.safe_load, instantiated UNCHANGED (minus ckpt_path) through util.instantiate_from_config, and every UNet / VQGAN
    state-dict key and shape must equal the enumeration the oracle and the synthetic-weight recipe are built on; the
    hyper-parameter copies in oracle/weights.py and dsml_thesis_amd/synth.py must equal the YAML's."""
    import os
    from dsml_thesis_amd import synth
    from dsml_thesis_amd.util import instantiate_from_config, load_yaml_config
    cfg = _strip_ckpt(load_yaml_config(os.path.join(GOLDEN, "configs", _YAMLS[which])))["model"]
    params = cfg["params"]
    ucfg, fcfg = params["unet_config"]["params"], params["first_stage_config"]["params"]
    want_unet = W.TF_UNET if which == "tf" else W.FR_UNET
    for table, name in ((want_unet, "oracle.weights"), (synth.TF_UNET if which == "tf" else synth.FR_UNET, "synth")):
        for k, v in table.items():
            assert ucfg[k] == v, (name, k, ucfg[k], v)
        assert set(ucfg) - set(table) <= {"use_checkpoint"}, (name, set(ucfg) - set(table))
    for table in (W.VQ_F4, synth.VQ_F4):
        assert fcfg["embed_dim"] == table["embed_dim"] and fcfg["n_embed"] == table["n_embed"]
        for k, v in table["ddconfig"].items():
            assert fcfg["ddconfig"][k] == v, (k, fcfg["ddconfig"][k], v)
    for table in (W.SCHEDULE, synth.SCHEDULE):
        assert {k: params[k] for k in table} == table
    model = instantiate_from_config(cfg)
    sd = model.state_dict()
    unet_keys = {"model.diffusion_model." + k: tuple(s) for k, s in W.unet_param_shapes(want_unet).items()}
    vq_keys = {"first_stage_model." + k: tuple(s) for k, s in W.vqmodel_param_shapes(W.VQ_F4).items()}
    for k, shp in {**unet_keys, **vq_keys}.items():
        assert tuple(sd[k].shape) == shp, k
    assert {k for k in sd if k.startswith("model.diffusion_model.")} == set(unet_keys)
    assert {k for k in sd if k.startswith("first_stage_model.")} == set(vq_keys)
    assert type(model).__name__ == {"fr": "LatentDiffusion", "fr_clip": "LatentDiffusionCLIP", "tf": "LatentDiffusion2Cond"}[which]
    assert model.num_timesteps == 1000 and model.channels == 3 and model.image_size == 32


def test_posterior_helpers_carry_the_reference_formulas():
    """LatentDiffusion.q_mean_variance / predict_start_from_noise / q_posterior (ddpm.py:203-228) are host-visible elementwise
    work on the registered schedule buffers (no kernel): against the oracle's schedule tables and its p_sample update
    (oracle.ddpm_update = predict_start_from_noise -> q_posterior -> mean + sigma z, ddpm.py:1049-1109)."""
    from helpers import fr_config
    from dsml_thesis_amd.ddpm import LatentDiffusion
    from oracle import ldm_oracle as O
    m = LatentDiffusion(**fr_config(unet=dict(W.FR_UNET, model_channels=32, channel_mult=[1], attention_resolutions=[1])))
    sched = O.register_schedule(**W.SCHEDULE)
    rs = np.random.RandomState(5)
    x, eps, nz = (torch.from_numpy(rs.standard_normal((3, 3, 8, 8)).astype(np.float32)) for _ in range(3))
    t = torch.tensor([0, 417, 999])
    g = lambda name: sched[name].gather(-1, t).reshape(3, 1, 1, 1)
    x0 = m.predict_start_from_noise(x, t, eps)
    assert torch.equal(x0, g("sqrt_recip_alphas_cumprod") * x - g("sqrt_recipm1_alphas_cumprod") * eps)
    mean, var, logvar = m.q_posterior(x0, x, t)
    assert mean.shape == x.shape and var.shape == (3, 1, 1, 1) and torch.equal(logvar, g("posterior_log_variance_clipped"))
    assert torch.equal(var, g("posterior_variance"))
    nonzero = (1 - (t == 0).float()).reshape(3, 1, 1, 1)
    assert torch.equal(mean + nonzero * (0.5 * logvar).exp() * nz, O.ddpm_update(sched, x, eps, t, nz))
    qm, qv, qlv = m.q_mean_variance(x, t)
    assert torch.equal(qm, g("sqrt_alphas_cumprod") * x) and torch.equal(qv, 1.0 - g("alphas_cumprod"))
    torch.testing.assert_close(qlv, torch.log(qv), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(m.q_sample(x, t, nz), qm + qv.sqrt() * nz, rtol=1e-6, atol=1e-6)      # (q_sample draws from that q)


def test_every_environment_switch_is_registered_and_documented():
    """dsml_thesis_amd/switches.py is the one table of `LDMK_*` environment switches: every read in the package goes through
    switches.get (no raw os.environ read of an LDMK_ name is left), with the default the table documents; every getenv in the
    library's sources and every read in bench.py names a registered switch -- the library's own switches through its one table
    (csrc/ldmk_common.h), with the defaults documented here; the table names nothing that is no longer read; every entry states
    its contract ("bits", "tolerance" or None); and docs/SWITCHES.md is the table's own rendering."""
    import glob
    import os
    import re
    from dsml_thesis_amd import switches as S
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    seen = set()
    for path in sorted(glob.glob(os.path.join(root, "dsml_thesis_amd", "*.py"))):
        src = open(path).read()
        if not path.endswith("switches.py"):
            assert not re.search(r'os\.environ(\.get\(|\[)\s*"LDMK_', src), f"raw environment read of an LDMK_ switch in {path}"
        for name, default in re.findall(r'switches\.get\("(LDMK_[A-Z0-9_]+)"(?:,\s*"([^"]*)")?\)', src):
            assert name in S.SWITCHES, (name, path)
            seen.add(name)
            table_default = S.SWITCHES[name][0]
            assert (default or None) == (table_default or None), (name, path, default, table_default)
    from dsml_thesis_amd import engine
    for name in engine._SECTIONS.values():                 # (read under a computed name: engine.table)
        assert name in S.SWITCHES, name
        seen.add(name)
    for path in sorted(glob.glob(os.path.join(root, "dsml_thesis_amd", "*.py"))):      # no environment read under a computed name is left raw
        if not path.endswith(("switches.py", "build.py")):
            assert "os.environ" not in open(path).read(), f"raw environment access in {path}"
    for path in sorted(glob.glob(os.path.join(root, "dsml_thesis_amd", "csrc", "*"))):
        if path.endswith((".hip", ".h")):
            for name in re.findall(r'getenv\("(LDMK_[A-Z0-9_]+)"\)', open(path).read()):
                assert name in S.PROBE_ONLY or S.SWITCHES.get(name, (None, None))[1] == "library", (name, path)
                seen.add(name)
    # the library's own switches: ONE table ({"LDMK_X", default, ...} in csrc/ldmk_common.h, read by getenv(e.name)), with the table's
    # defaults (unset = 0 there); no other source reads a library switch by itself
    common = open(os.path.join(root, "dsml_thesis_amd", "csrc", "ldmk_common.h")).read()
    assert "getenv(e.name)" in common
    lib_table = dict(re.findall(r'\{"(LDMK_[A-Z0-9_]+)",\s*(-?\d+),', common))
    assert set(lib_table) == {n for n, v in S.SWITCHES.items() if v[1] == "library"}, sorted(lib_table)
    for name, default in lib_table.items():
        assert int(default) == int(S.SWITCHES[name][0] or 0), (name, default)
        assert name not in seen, f"{name} is read outside the library's switch table"
        seen.add(name)
    for name, entry in S.SWITCHES.items():
        assert len(entry) == 4 and entry[3] in ("bits", "tolerance", None), (name, entry)
        assert entry[3] is None or entry[1] in ("arithmetic", "route", "library"), (name, entry)
        assert entry[1] != "library" or entry[3] is not None, f"{name}: a library switch is an A/B arm and states its contract"
    for name in re.findall(r'os\.environ\.get\("(LDMK_[A-Z0-9_]+)"', open(os.path.join(root, "bench.py")).read()):
        assert name in S.SWITCHES, (name, "bench.py")
        seen.add(name)
    stale = set(S.SWITCHES) - seen
    assert not stale, f"registered but never read: {sorted(stale)}"
    with pytest.raises(KeyError):
        S.get("LDMK_NOT_A_SWITCH")
    assert open(os.path.join(root, "docs", "SWITCHES.md")).read().strip() == S.table_markdown().strip()


def test_sampler_conditioning_forms():
    """DDIMSampler._split_cond (host logic, no kernel): every form the reference's apply_model accepts (ddpm.py:893-994) maps to
    (cross-attention context, channel concat) -- or, for conditioning_key 'adm', to the class-label vector (ddpm.py:1417-1419)."""
    from dsml_thesis_amd.ddim import DDIMSampler, C12, C34

    class Wrapper:
        conditioning_key = "crossattn"

    class Model:
        num_timesteps = 1000
        device = torch.device("cpu")
        model = Wrapper()
    s = DDIMSampler(Model())
    ctx, cat, y = torch.zeros(2, 1, 512), torch.zeros(2, 6, 8, 8), torch.tensor([7, 2])
    assert s._split_cond(ctx)[0] is ctx and s._split_cond(ctx)[1] is None
    assert s._split_cond([ctx, ctx])[0].shape == (2, 2, 512)                    # lists are concatenated on the token axis
    a, b = s._split_cond({"c_crossattn": [ctx], "c_concat": [cat, cat]})
    assert a.shape == (2, 1, 512) and b.shape == (2, 12, 8, 8)
    a, b = s._split_cond({C12: ctx, C34: cat})                                  # the talking-face sampler's dict (ddim2cond.py:165)
    assert a is ctx and b is cat
    assert s._split_cond(None) == (None, None)
    Wrapper.conditioning_key = "concat"
    assert s._split_cond(cat)[0] is None and s._split_cond(cat)[1] is cat
    Wrapper.conditioning_key = "adm"
    for form in (y, [y], {"c_crossattn": [y]}):
        lab, none = s._split_cond(form)
        assert lab is y and none is None


def test_bench_dump_outputs_budget_and_fixed_sample(tmp_path, monkeypatch):
    """bench.py --dump-outputs: float32 .npy per array; an array over its share of the byte budget is written as a seeded
    sample, the same one every time, and the files stay within the budget."""
    import os
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 64 * 1024)
    small = torch.arange(12, dtype=torch.float64).reshape(3, 4)
    big = torch.randn(100_000, generator=torch.Generator().manual_seed(0))
    for d in ("a", "b"):
        bench.save_outputs(str(tmp_path / d), {"small": small, "big": big})
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and s.shape == (3, 4) and np.array_equal(s, small.numpy().astype(np.float32))
    b = np.load(tmp_path / "a" / "big.npy")
    assert b.dtype == np.float32 and 0 < b.size <= bench.DUMP_BYTES // 8 and np.isin(b, big.numpy()).all()
    assert np.array_equal(b, np.load(tmp_path / "b" / "big.npy"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= bench.DUMP_BYTES
