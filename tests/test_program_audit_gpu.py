"""GPU: the recorded launch programs themselves (tests/program_audit.py): buffer lifetimes, extents, stale and unwritten reads.

Every inference path is recorded once into an engine.Program whose arguments are raw device pointers and whose scratch comes from a
free list keyed by the exact element count, returned by hand.  The other tests see eps or an image at a fixture shape, where a
buffer released one call early, a pointer to a dead temporary, a read of memory nothing wrote or a buffer a little short gives
finite, plausible numbers.  Here each program is built twice -- as shipped, and under the recorder with nothing recycled -- and
held to

  static (no launch; true for every shape the same builder code takes)
    R1 no call holds a pointer into a buffer released before it      R2 no double / foreign / partial-view release, no stale
    R3 inputs, outputs and the context program's buffers stay           GroupNorm record behind a direct Program.release
    R4 every other pointer lies in a block a live tensor owns        R5 every pointer's extent (include/ldmk.h) fits its buffer
  dynamic (2 x 32 x 32 or smaller, programs driven directly so that the test owns the workspace)
    D1 pooled == unpooled, same launches      D2 0xFF in every workspace byte changes nothing and raises no flag
    D3 inputs A, B, A: the third output is the first

All comparisons are set memberships, integer inequalities or torch.equal.  CASES is the matrix; the coverage test at the end
fails when a `.release(` call site of the product files ran in none of its builds."""
import contextlib
import ctypes as C
import json
import os
import tempfile

import pytest
import torch

import program_audit as A
from conftest import rnd
from oracle import weights as W

pytestmark = pytest.mark.gpu

THRESHOLDS = {  # module attribute a case may lower (as tests/test_switch_arms_model_gpu.py does) -> where it lives
    "ATTN_PRESPLIT_MIN_TOKENS": "unet", "ATTN_H2_MIN_TOKENS": "unet", "WINO_MIN_TILES": "NetBuilder", "WINO_MIN_CIN": "NetBuilder",
    "UP_MIN_PIXELS": "NetBuilder",
}
WINO = dict(WINO_MIN_TILES=1, UP_MIN_PIXELS=1)


def U(cfg="FR_UNET", policy=16, n=2, hw=32, L_ctx=1, cc=0, env=None, attrs=None, deny=False, gain=1.0, plans=None):
    return dict(kind="unet", cfg=cfg, policy=policy, n=n, hw=hw, L_ctx=L_ctx, cc=cc, env=env or {}, attrs=attrs or {}, deny=deny, gain=gain,
                plans=plans or {})


def FS(model, prog, n, hw, quantize=None, env=None, attrs=None):
    return dict(kind="fs", model=model, prog=prog, n=n, hw=hw, quantize=quantize, env=env or {}, attrs=attrs or {}, plans={})


# Two branches are behind plan-table entries the shipped igemm_plans.json does not hold; a case reaches them the supported way, with
# a plan file of its own for ONE section (LDMK_PLAN_TABLE / LDMK_PS_TABLE, engine._SECTIONS): the shipped section plus these entries.
#  * unet_small.py: the small route's GEGLU projection on a slab GEMM that splits K (raw slabs, summed by ldmk_post).  The C++
#    heuristic never splits a GEGLU product and the shipped "f32" section lists no such plan; tests/test_small_batch_gpu.py runs
#    the kernel pair (tile_cfg 14, raw slabs, geglu post) on its own.  Keys: the 16 x 16 and 8 x 8 levels of the 2 x 32 x 32 job.
GEGLU_SLAB_SPLIT = {"f32": lambda shipped: {"512,2560,320,0,0,1,1": [14, 2], "128,5120,640,0,0,1,1": [14, 2]}}
#  * engine.py gn_conv / up_conv and unet.py attn1: the Winograd planes, the upsampling phases and the attention result written in
#    the THREE-plane bf16 form of the PS layout (ldmk_winograd_input_ps, ldmk_upconv_gather_ps, ldmk_attn_self_x3p_ps).  The
#    shipped "ps_bf16x3" section lists nine shapes, none of them batched and no attn1.to_out (those all moved to the F16X2 form);
#    the tiles of "ps_f16x2" (23..28, 31..33) are tiles of both forms (include/ldmk.h), and Program.igemm_ps checks each plan.
PS_X3_PLANES = {"ps_bf16x3": lambda shipped: {k: v for k, v in shipped["ps_f16x2"].items() if k not in shipped["ps_bf16x3"]}}


CASES = {
    # ---- the FR UNet at 2 x 32 x 32 with the plans of each BASELINE batch; 1 and 3 context tokens; the talking-face concat (g7)
    "fr_small": U(policy=None), "fr_p16": U(policy=16), "fr_p64": U(policy=64), "fr_p128": U(policy=128),
    "fr_p16_L3": U(policy=16, L_ctx=3), "fr_p128_L3": U(policy=128, L_ctx=3), "fr_none_L3": U(policy=None, L_ctx=3),
    "tf_small": U("TF_UNET", policy=None, cc=6), "tf_p16": U("TF_UNET", policy=16, cc=6), "tf_p128": U("TF_UNET", policy=128, cc=6),
    # ---- every switch that changes which builder code runs
    "no_ps": U(env={"LDMK_PS": "0"}), "no_psc": U(env={"LDMK_PSC": "0"}), "no_winograd": U(env={"LDMK_NO_WINOGRAD": "1"}),
    "no_attn_ps": U(env={"LDMK_ATTN_PS": "0"}), "no_fold_pout": U(policy=64, env={"LDMK_FOLD_POUT": "0"}),
    "pout_ps": U(policy=64, env={"LDMK_FOLD_POUT": "0", "LDMK_POUT_PS": "1"}),
    "ln_unfolded": U(env={"LDMK_LN_UNFOLDED": "1"}), "ln_unfolded_L3": U(L_ctx=3, env={"LDMK_LN_UNFOLDED": "1"}),
    "no_qkv_tiles": U(env={"LDMK_QKV_TILES": "0"}), "no_f16x2": U(env={"LDMK_F16X2": "0"}), "no_split": U(env={"LDMK_SPLIT_BF16": "0"}),
    "no_small_route": U(policy=None, env={"LDMK_NO_SMALL_ROUTE": "1"}), "splitk_in_launch": U(env={"LDMK_SPLITK_IN_LAUNCH": "1"}),
    # ---- thresholds lowered until every branch of emit_self_attention, gn_conv and up_conv is emitted
    "presplit": U(attrs={"ATTN_PRESPLIT_MIN_TOKENS": 1}), "presplit_x3": U(env={"LDMK_F16X2": "0"}, attrs={"ATTN_PRESPLIT_MIN_TOKENS": 1}, plans=PS_X3_PLANES),
    "presplit_x3_no_attn_ps": U(env={"LDMK_F16X2": "0", "LDMK_ATTN_PS": "0"}, attrs={"ATTN_PRESPLIT_MIN_TOKENS": 1}),
    "no_presplit": U(env={"LDMK_ATTN_PRESPLIT": "0"}, attrs={"ATTN_PRESPLIT_MIN_TOKENS": 1}),
    "h2_everywhere": U(attrs={"ATTN_H2_MIN_TOKENS": 1}), "h2_everywhere_no_tiles": U(env={"LDMK_QKV_TILES": "0"}, attrs={"ATTN_H2_MIN_TOKENS": 1}),
    "h2_no_tiles_no_attn_ps": U(env={"LDMK_QKV_TILES": "0", "LDMK_ATTN_PS": "0"}, attrs={"ATTN_H2_MIN_TOKENS": 1}),
    "wino": U(env={"LDMK_PSC": "0"}, attrs=WINO), "wino_no_ps": U(env={"LDMK_PSC": "0", "LDMK_PS": "0"}, attrs=WINO),
    "wino_x3": U(env={"LDMK_PSC": "0", "LDMK_F16X2": "0"}, attrs=WINO, plans=PS_X3_PLANES),
    "small_geglu_split": U(policy=None, plans=GEGLU_SLAB_SPLIT), "wino_narrow": U(env={"LDMK_PSC": "0"}, attrs=dict(WINO, WINO_MIN_CIN=1)),
    "wino_f32": U(env={"LDMK_PSC": "0", "LDMK_SPLIT_BF16": "0"}, attrs=WINO),
    # ---- the UNet variants of g14 / g15
    "h40": U("H40_UNET", policy=None, hw=16), "h40_L3_p16": U("H40_UNET", policy=16, hw=16, L_ctx=3), "h64": U("H64_UNET", policy=16, hw=16),
    "adm": U("ADM_UNET", policy=None, hw=16, L_ctx=0), "adm_p16": U("ADM_UNET", policy=16, hw=16, L_ctx=0),
    "uncond": U("UNCOND_UNET", policy=None, L_ctx=0, gain=0.25), "uncond_p16": U("UNCOND_UNET", policy=16, L_ctx=0, gain=0.25),
    "updown": U("UPDOWN_UNET", policy=16), "updown_small": U("UPDOWN_UNET", policy=None), "updown_adm": U("UPDOWN_ADM_UNET", policy=16, hw=16, L_ctx=0),
    # ---- mixed arithmetic: some sites denied F16X2
    "denied_sites": U(deny=True), "denied_sites_p128": U(policy=128, deny=True),
    # ---- first stages: VQ decode with / without the lookup, VQ encode, the decoder's AttnBlock (mid.attn_1), KL, crops as batch items
    "vq_decode": FS("vq", "dec", 1, 16, True), "vq_decode_unquantised": FS("vq", "dec", 1, 16, False), "vq_encode": FS("vq", "enc", 1, 64),
    "vq_decode_crops": FS("vq", "dec", 4, 8, True), "vq_decode_wino": FS("vq", "dec", 1, 16, True, attrs=WINO),
    "kl_encode": FS("kl", "enc", 1, 64), "kl_decode": FS("kl", "dec", 2, 8, False),
}


@contextlib.contextmanager
def configured(env, attrs, plans, tmp):
    """the case's switches in the environment, its thresholds in the module attributes and its plan file (if any) behind the
    section's switch; plan tables reloaded on both sides"""
    from dsml_thesis_amd import engine, unet
    owner = {"unet": unet, "NetBuilder": engine.NetBuilder}
    env = dict(env)
    for section, extra in plans.items():
        with open(engine._PLAN_FILE) as f:
            shipped = json.load(f)
        path = os.path.join(tmp, f"{section}.json")
        with open(path, "w") as f:
            json.dump(dict(shipped[section], **extra(shipped)), f)
        env[engine._SECTIONS[section]] = path
    old_env = {k: os.environ.get(k) for k in env}
    old_attr = {k: getattr(owner[THRESHOLDS[k]], k) for k in attrs}
    try:
        os.environ.update(env)
        for k, v in attrs.items():
            setattr(owner[THRESHOLDS[k]], k, v)
        engine.reset_tables()
        yield
    finally:
        for k, v in old_env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        for k, v in old_attr.items():
            setattr(owner[THRESHOLDS[k]], k, v)
        engine.reset_tables()


class UNetSubject:
    def __init__(self, c):
        from test_unet_gpu import make_unet
        self.c = c
        self.cfg = getattr(W, c["cfg"])
        self.m, _ = make_unet(self.cfg, gain=c["gain"])
        self.m.policy_batch = c["policy"]
        if c["deny"]:          # a first build registers the sites; every third one then goes to bf16x3 and the programs are rebuilt
            self.build()
            names = sorted(self.m._sites.index)
            assert len(names) >= 9
            self.m.deny_f16x2(names[::3])

    def build(self):
        c = self.c
        self.m._programs.clear()
        pg = self.m.program(c["n"], c["hw"], c["hw"], c["L_ctx"], c["cc"])
        self.m._programs.clear()          # (no audited program stays cached for another test)
        return pg

    def inputs(self, seed):
        c, cfg = self.c, self.cfg
        n, hw = c["n"], c["hw"]
        d = dict(x=rnd(41 + seed, n, cfg["in_channels"] - c["cc"], hw, hw), t=torch.tensor([[3, 981], [500, 17]][seed % 2][:n]))
        if c["L_ctx"]:
            d["context"] = rnd(42 + seed, n * c["L_ctx"], cfg["context_dim"])
        if c["cc"]:
            d["c_concat"] = rnd(73 + seed, n, c["cc"], hw, hw)
        if cfg.get("num_classes"):
            d["y_emb"] = self.m.label_emb.weight.detach().float()[torch.tensor([[7, 2], [0, 9]][seed % 2][:n]).cuda()]
        return d

    def flags(self):
        st = self.m.arithmetic_status()
        return set(st["flags_up"]) | ({"<layernorm guard>"} if st["ln_flag_up"] else set())


class FirstStageSubject:
    def __init__(self, c):
        from dsml_thesis_amd import synth
        from dsml_thesis_amd.autoencoder import AutoencoderKL
        self.c = c
        if c["model"] == "vq":
            self.m = synth.make_vq_first_stage(synth.VQ_F4)
        else:
            kl = synth.KL_F4
            self.m = AutoencoderKL(ddconfig=dict(kl["ddconfig"]), lossconfig=dict(target="torch.nn.Identity"), embed_dim=kl["embed_dim"])
            synth.load_recipe(self.m)
            self.m = self.m.cuda().eval()

    def build(self):
        c = self.c
        self.m._programs.clear()
        key = (c["n"], c["hw"], c["hw"]) + ((c["quantize"],) if c["prog"] == "dec" else ())
        pg = self.m._program(c["prog"], *key)
        self.m._programs.clear()
        return pg

    def inputs(self, seed):
        c = self.c
        if c["prog"] == "dec":
            return dict(z=rnd(61 + seed, c["n"], self.m.embed_dim, c["hw"], c["hw"]))
        return dict(x=torch.tanh(rnd(64 + seed, c["n"], 3, c["hw"], c["hw"])))

    def flags(self):
        return set()


_RESULTS = {}


def run_case(name):
    """Build, drive and audit one case, once per session: the coverage test reads every case's release sites."""
    if name in _RESULTS:
        return _RESULTS[name]
    c = CASES[name]
    r = {}
    with tempfile.TemporaryDirectory() as tmp, configured(c["env"], c["attrs"], c["plans"], tmp):
        s = UNetSubject(c) if c["kind"] == "unet" else FirstStageSubject(c)
        a, b = s.inputs(0), s.inputs(1)
        pooled = s.build()
        first = A.drive(pooled, a)
        flags0 = s.flags()
        r["finite"] = A.finite(first)
        # D2: every workspace byte 0xFF before the inputs go in.  Exempt (program_audit.poison), and nothing else: pooled._skcnt and
        # pooled.ctx_program._skcnt, the arrival counters of the in-launch split-K combine, which engine.Program.splitk_counters
        # creates zeroed -- `self._skcnt = torch.zeros(n, device=self.device, dtype=torch.int32)` -- and every launch leaves zeroed
        A.poison(pooled)
        poisoned = A.drive(pooled, a)
        r["d2"] = A.finite(poisoned) and A.same(first, poisoned)
        r["d2_flags"] = sorted(s.flags() - flags0)
        # D3: A, B, A
        A.drive(pooled, b)
        r["d3"] = A.same(first, A.drive(pooled, a))
        # the same program under the recorder: nothing recycled
        with A.Recorder() as rec:
            unpooled = s.build()
        r["report"] = A.audit(rec, unpooled)
        r["d1_names"] = [k[3] for k in pooled.calls] == [k[3] for k in unpooled.calls] and (
            [k[3] for k in pooled.ctx_program.calls] == [k[3] for k in unpooled.ctx_program.calls] if hasattr(pooled, "ctx_program") else True)
        r["d1"] = A.same(first, A.drive(unpooled, a))
        r["release_lines"] = rec.release_lines
        r["names"] = {k[3] for k in unpooled.calls}
        r["bytes"] = (pooled.workspace_bytes(), unpooled.workspace_bytes())
        r["buffers"] = len(rec.buffers)
    _RESULTS[name] = r
    return r


@pytest.mark.parametrize("name", list(CASES))
def test_program(name):
    r = run_case(name)
    rep = r["report"]
    print(f"{name}: {rep.calls} calls, {rep.pointers} pointer arguments checked, {r['buffers']} buffers; workspace pooled "
          f"{r['bytes'][0]} / unpooled {r['bytes'][1]} bytes")
    assert rep.pointers > 0 and r["finite"]
    assert not rep.findings, f"static audit of {name}: {rep}"
    assert r["d1_names"], "D1: the program built under the recorder is not the shipped program (launch names differ)"
    assert r["d1"], "D1: the pool changes the result (pooled != unpooled)"
    assert r["d2"], "D2: 0xFF in the workspace changes the result: a kernel reads memory that no call of the program wrote"
    assert not r["d2_flags"], f"D2: garbage in the workspace raised {r['d2_flags']} (a full repeat in bf16x3, and a result that depends on history)"
    assert r["d3"], "D3: the result depends on what the workspace held from an earlier run (A, B, A: third != first)"


def test_what_the_pool_buys():
    """on record, not asserted: the workspace of the FR UNet at policy 16 with and without recycling"""
    r = run_case("fr_p16")
    print(f"FR UNet 2 x 32 x 32, policy_batch 16: workspace_bytes() pooled {r['bytes'][0]}, unpooled {r['bytes'][1]} "
          f"({r['bytes'][1] / r['bytes'][0]:.2f} x)")


def test_the_matrix_reaches_every_route():
    """what the cases are for: each route's launches appear in the build that is meant to emit them"""
    names = lambda k: run_case(k)["names"]
    assert "ldmk_post" in names("fr_small") and "ldmk_post" not in names("no_small_route")
    assert names("small_geglu_split") == names("fr_small")          # (the same launches: what differs is the GEGLU GEMM's plan)
    assert "ldmk_attn_cross" in names("fr_p16_L3") and "ldmk_attn_cross_d" in names("h40_L3_p16")
    assert "ldmk_gn_apply_ps_h2" in names("fr_p16") and "ldmk_gn_apply_ps_h2" not in names("no_psc")
    assert "ldmk_winograd_input_ps_h2" in names("wino") and "ldmk_upconv_gather_ps_h2" in names("wino")
    assert "ldmk_winograd_input_ps" in names("wino_x3") and "ldmk_upconv_gather_ps" in names("wino_x3")
    assert "ldmk_winograd_input" in names("wino_no_ps") and "ldmk_upconv_gather" in names("wino_no_ps")
    assert "ldmk_attn_self_h2_tiles" in names("fr_p16") and "ldmk_attn_self_h2_tiles" not in names("no_qkv_tiles")
    assert "ldmk_attn_self_h2_ps" in names("no_qkv_tiles") and "ldmk_attn_self_h2" in names("h2_no_tiles_no_attn_ps")
    assert "ldmk_attn_self_x3p_ps" in names("presplit_x3") and "ldmk_attn_self_x3p" in names("presplit_x3_no_attn_ps")
    assert "ldmk_attn_self_x3" in names("no_presplit") and "ldmk_attn_self" in names("no_split")
    assert "ldmk_ln_stats" in names("ln_unfolded") and "ldmk_heads_gather" in names("h40") and "ldmk_gn_coef_film" in names("adm")
    assert "ldmk_resample2" in names("updown") and "ldmk_vq_nearest" in names("vq_decode") and "ldmk_vq_nearest" not in names("vq_decode_unquantised")
    assert "ldmk_conv3x3_moments" in names("kl_encode") and "ldmk_softmax_rows" in names("vq_decode")


# `.release(` call sites that no supported configuration reaches: (file, the call's source text) -> why
EXCLUDED = {}


def test_every_release_site_ran_in_an_audited_build():
    lines = set()
    pointers = 0
    for name in CASES:
        r = run_case(name)
        lines |= r["release_lines"]
        pointers += r["report"].pointers
    sites = A.release_call_sites()
    assert len(sites) >= 50
    missing = [s for s in sites if not A.executed(s, lines) and (s[0], s[3]) not in EXCLUDED]
    print(f"{len(sites)} release call sites, {len(sites) - len(missing)} executed; {pointers} pointer arguments checked in {len(CASES)} programs")
    assert not missing, "release sites that ran in no audited build (add the configuration that reaches them): " + "; ".join(
        f"{f}:{lo} `{src}`" for f, lo, _, src in missing)
    stale = [k for k in EXCLUDED if not any((s[0], s[3]) == k for s in sites)]
    assert not stale, f"EXCLUDED names call sites that no longer exist: {stale}"


# ---------------------------------------------------------------------------------------------- the audit fails when it should
# Tiny hand-built programs (1024-float buffers; ldmk_silu, ldmk_axpy, one 64 x 64 x 64 ldmk_igemm) with ONE seeded violation each.
# They are audited, never run -- except the read-before-write one, which stays in bounds.
N = 1024


def _tiny(dev="cuda"):
    from dsml_thesis_amd.engine import Program
    return Program(dev)


def _gemm(pg, out=None, stats=None, splitk=1, ws=None, dev="cuda"):
    """one planned 64 x 64 x 64 GEMM, recorded as unet_small records its pinned ones; -> (args, the tensors it needs alive)"""
    from dsml_thesis_amd import ops
    a0 = pg.alloc(64, 64)
    w = torch.zeros(64, 64, device=dev)
    out = pg.alloc(64, 64) if out is None else out
    a = ops.make_igemm_args(64, 64, 64, a0, 64, w, out, 64, 64)
    a.tile_cfg, a.splitk = 1, splitk
    if stats is not None:
        a.stats_out = stats.data_ptr()
    if ws is not None:
        a.splitk_ws, a.splitk_ws_elems = ws.data_ptr(), ws.numel()
    pg.calls.append((pg.lib.ldmk_igemm, (C.byref(a),), a, "ldmk_igemm"))
    return a, (w,)


def seeded(kind, dev="cuda"):
    """-> (recorder, program, tensors to keep alive)"""
    x = torch.zeros(N, device=dev)
    keep = [x]
    with A.Recorder() as rec:
        pg = _tiny(dev)
        a, b = pg.alloc(N), pg.alloc(4, N // 4)
        pg.add("ldmk_silu", x.data_ptr(), a.data_ptr(), N)
        pg.add("ldmk_silu", a.data_ptr(), b.data_ptr(), N)
        if kind == "clean":
            pg.release(a)
            ws = pg.alloc(2 * 64 * 64)
            keep += [_gemm(pg, stats=pg.alloc(2, 64, 3), dev=dev), _gemm(pg, splitk=2, ws=ws, dev=dev)]
        elif kind == "read after release":
            pg.release(a)
            pg.add("ldmk_axpy", b.data_ptr(), a.data_ptr(), 1.0, N)
        elif kind == "double release":
            pg.release(a)
            pg.release(a)
        elif kind == "interior view":
            pg.release(b[1:])
        elif kind == "ctx_program buffer":
            ctx = _tiny(dev)
            v = ctx.alloc(N)
            ctx.add("ldmk_silu", x.data_ptr(), v.data_ptr(), N)
            ctx.release(v)
            pg.ctx_program = ctx
        elif kind == "deleted tensor":
            t = torch.zeros(N, device=dev)
            pg.add("ldmk_axpy", b.data_ptr(), t.data_ptr(), 1.0, N)
            del t
        elif kind == "out one row short":
            keep.append(_gemm(pg, out=pg.alloc(63, 64), dev=dev))
        elif kind == "stats_out one record short":
            keep.append(_gemm(pg, stats=pg.alloc(2 * 64 * 3 - 3), dev=dev))
        elif kind == "split-K scratch too small":
            keep.append(_gemm(pg, splitk=2, ws=pg.alloc(2 * 64 * 64 - 64), dev=dev))
        else:
            raise AssertionError(kind)
    return rec, pg, keep


SEEDED = {"clean": [], "read after release": ["R1"], "double release": ["R2"], "interior view": ["R2"], "ctx_program buffer": ["R3"],
          "deleted tensor": ["R4"], "out one row short": ["R5"], "stats_out one record short": ["R5"], "split-K scratch too small": ["R5"]}


@pytest.mark.parametrize("kind", list(SEEDED))
def test_a_seeded_violation_is_reported_by_its_rule_and_only_by_it(kind):
    rec, pg, keep = seeded(kind)
    rep = A.audit(rec, pg)
    print(f"{kind}: {rep}")
    assert rep.rules() == SEEDED[kind], str(rep)
    assert len(rep.findings) == len(SEEDED[kind]), str(rep)
    if kind == "split-K scratch too small":
        assert "needs 8192 floats, the call offers 8128" in rep.findings[0].message
    if kind == "clean":
        assert rep.pointers >= 12


def test_a_read_before_write_fails_the_poisoned_run():
    """The one seeded program that runs: axpy onto the output from a buffer nothing wrote.  In bounds; the static rules have nothing
    to say about it; D2 does."""
    with A.Recorder() as rec:
        pg = _tiny()
        x, never, y = pg.alloc(N), pg.alloc(N), pg.alloc(N)
        pg.inputs, pg.outputs = dict(x=x), dict(y=y)
        pg.add("ldmk_silu", x.data_ptr(), y.data_ptr(), N)
        pg.add("ldmk_axpy", y.data_ptr(), never.data_ptr(), 1.0, N)
    assert not A.audit(rec, pg).findings
    never.zero_()
    first = A.drive(pg, dict(x=rnd(7, N)))
    assert A.finite(first)
    A.poison(pg)
    poisoned = A.drive(pg, dict(x=rnd(7, N)))
    assert not A.finite(poisoned) and not A.same(first, poisoned)


def test_the_unquantised_decode_offers_no_indices():
    """Found by D2: the decode program without the codebook lookup listed an `indices` output that no launch writes (whatever the
    pool buffer held); it has none now, and asking for indices there is an error instead of garbage."""
    from dsml_thesis_amd import lib as L
    s = FirstStageSubject(CASES["vq_decode_unquantised"])
    assert set(s.build().outputs) == {"image"}
    assert set(FirstStageSubject(CASES["vq_decode"]).build().outputs) == {"image", "indices"}
    with pytest.raises(L.LdmkError, match="return_indices"):
        s.m.decode(rnd(61, 1, 3, 16, 16).cuda(), force_not_quantize=True, return_indices=True)
