"""Record what engine.Program.plan decides for every tuned shape under every planning input, without a GPU.

    python tools/record_plan_decisions.py [OUT.json]        (default: tests/golden/plan_decisions.json)

ldmk_igemm_check / ldmk_igemm_plan are host code, so the whole decision -- arithmetic, tile, K split, which weight images, whether
a pre-split A survives -- can be pinned on any machine.  tests/test_plan_selection.py rebuilds the cases below and compares
Program.plan against the recorded file, which is made by running THIS script on the commit whose behaviour is to be kept.

A case = a key of the plan file ("M,N,K,a_mode,a_tf,epi,batch[,bt][,s<stride>u<upsample>]", every key of the f32 / bf16x3 / f16x2
sections) x a variant (the full cross of VARIANT_AXES).  The args carry dummy non-null pointers: validation precedes any launch.
Weight images are registered by hand against a CPU tensor standing in for the weight, with the ld the packers would give them.

File: {"fields", "variants" (count), "cases" (count), "shapes": {rest of the key after M: digest}, "classes": {outcome class:
[count, example key, example variant]}}.  A digest is the first 16 hex digits of the SHA-256 of the shape's keys (by rising M) and the
`fields` values every variant of each left in the args, in order -- half a million outcomes are compared through some 300 lines.
`--dump SHAPE` prints those outcomes instead, to diff two trees by hand when a digest differs.
"""
import ctypes as C
import hashlib
import itertools
import json
import os
import sys
import weakref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from dsml_thesis_amd import engine, ops  # noqa: E402
from dsml_thesis_amd import lib as L  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "plan_decisions.json")
SECTIONS = ("f32", "bf16x3", "f16x2")
# what Program.plan may write, as compared after the call (pointers as "set / not set")
FIELDS = ("M", "batch", "tile_cfg", "splitk", "splitk_ws", "splitk_ws_elems", "compute", "w_split", "w_split_ld", "w_split_bstride",
          "w_scale_exp", "range_flag", "a_split", "a_split_ld", "raw_slabs")
_AS_BOOL = ("w_split", "range_flag", "a_split")
# rows: "tuned" = the key's M; "eighth" = an eighth of it, planned with scale_m = (8, 1); "triple" = three times it.  (The axes are
# ordered so that the outcome changes as rarely as possible from one variant to the next: the file stores runs.)
VARIANT_AXES = (("rows", ("tuned", "eighth", "triple")),
                ("alt_batch", (False, True)),      # batch > 1: batch_is_samples False / True; batch == 1: per_sample False / True
                ("allow_splitk", (True, False)), ("a_split", (False, True)), ("images", ("none", "x3", "both")),
                ("flag", (False, True)), ("far", (False, True)), ("w_frag", (True, False)))
_NAMES = tuple(n for n, _ in VARIANT_AXES)
VARIANTS = [dict(zip(_NAMES, v)) for v in itertools.product(*(vals for _, vals in VARIANT_AXES))]
# ... and beside the full cross: a shard of a job eight times as large as three times the tuned row count, where the POLICY problem
# outgrows the 32-bit offsets of the largest shapes while the real one does not
VARIANTS += [dict(zip(_NAMES, ("triple_eighth", False, True, False, im, fl, far, True)))
             for im in ("none", "x3", "both") for fl in (False, True) for far in (False, True)]
CLASSES = ("f16x2_from_its_section", "f16x2_via_x3_key_21_to_5", "f16x2_via_x3_key_22_to_1", "long_k_conv_rule_tuned_f32_plan",
           "long_k_conv_rule_heuristic_plan", "bf16x3_lds_tile_a_split_kept", "bf16x3_ws_tile_a_split_dropped",
           "split_plan_legal_for_real_not_policy_problem", "row_or_slab_tile_accepted", "row_or_slab_tile_no_w_frag",
           "row_or_slab_tile_refused_for_real_problem", "plain_heuristic", "sample_batch_scales_batch")
# classes no case of the grid reaches with the plan file as it is (recorded with count 0; the test notices when that changes)
UNREACHABLE = {
    "f16x2_via_x3_key_21_to_5": "both bf16x3 entries on tile 21 are also listed in the f16x2 section at the same row counts, and that "
                                "section is asked first whenever the range flag is set",
    "row_or_slab_tile_refused_for_real_problem": "every row-count condition of ldmk_igemm_check is an upper bound and a shard never has "
                                                 "more rows than its job, so a tile legal for the policy problem is legal for the real one",
}
PTR = 4096                # a non-null "device pointer" that is never dereferenced
SCALE_EXP = 3
_W = torch.zeros(8)       # stands in for the weight: its address is what the image registry is keyed by
_IMG = torch.zeros(8)
_FLAG = torch.zeros(1, dtype=torch.int32)


def keys():
    """Every key of the three sections of the plan file, once (a shape listed in two sections is the same case)."""
    raw = json.load(open(engine._PLAN_FILE))
    return sorted({k for s in SECTIONS for k in raw[s]})


def _square(rows):
    """The largest power-of-two square image side whose pixel count divides `rows`."""
    return next(s for s in (64, 32, 16, 8, 4, 2, 1) if rows % (s * s) == 0)


def base_args(key):
    """IgemmArgs of the key's problem at its own M, every operand the shape needs present."""
    parts = key.split(",")
    M, N, K, mode, tf, epi, batch = (int(v) for v in parts[:7])
    a = L.IgemmArgs()
    a.M, a.N, a.K, a.a_mode, a.a_tf, a.epi, a.batch = M, N, K, mode, tf, epi, batch
    a.a0 = a.out = PTR
    a.w = _W.data_ptr()
    a.b_trans = 1 if "bt" in parts[7:] else 0
    a.ldb = K if a.b_trans else N
    a.ldc = N // 2 if epi == L.EPI_GEGLU else N
    if mode == L.A_CONV3X3:
        a.c0 = K // 9
        a.stride, a.pad_lo = 1, 1
        for p in parts[7:]:
            if p.startswith("s"):
                a.stride, a.upsample = (int(v) for v in p[1:].split("u"))
    else:
        a.c0 = K
    if tf in (L.TF_AFFINE, L.TF_AFFINE_SILU):
        a.tf_coef = PTR
    elif tf == L.TF_LAYERNORM:
        a.row_stats = a.ln_gamma = a.ln_beta = PTR
    elif tf == L.TF_LAYERNORM_FOLDED:
        a.row_stats = a.ln_colsum = PTR
    if batch > 1:
        a.a_bstride, a.w_bstride, a.out_bstride = M * K, K * N, M * N
    return a


def set_rows(a, rows):
    """The problem at `rows` rows: square images of the largest power-of-two side that divides the row count."""
    a.M = rows
    s = _square(rows)
    a.rows_per_sample = s * s
    if a.a_mode == L.A_CONV3X3:
        a.out_h = a.out_w = s
        a.in_h = a.in_w = max(1, s // 2) if a.upsample else s * a.stride


def register_images(which, N, K):
    """Put hand-made image records for _W into the registry (whatever form this tree's ops.py keeps it in)."""
    ld, ref, ver, p = (K + 7) // 8 * 8, weakref.ref(_W), _W._version, _W.data_ptr()
    x3, h2 = which in ("x3", "both"), which == "both"
    if hasattr(ops, "_SPLIT_H2"):          # two positional-tuple registries
        ops._SPLIT.pop(p, None)
        ops._SPLIT_H2.pop(p, None)
        if x3:
            ops._SPLIT[p] = (_IMG, ld, 3 * N * ld, ref, ver)
        if h2:
            ops._SPLIT_H2[p] = (_IMG, ld, 2 * N * ld, ref, ver, SCALE_EXP)
    else:                                  # one registry of named records
        ops._IMAGES.clear()
        if x3:
            ops._IMAGES[(p, L.COMPUTE_BF16X3)] = ops.WeightImage(_IMG, ld, 3 * N * ld, ref, ver, 0, L.COMPUTE_BF16X3)
        if h2:
            ops._IMAGES[(p, L.COMPUTE_F16X2)] = ops.WeightImage(_IMG, ld, 2 * N * ld, ref, ver, SCALE_EXP, L.COMPUTE_F16X2)


def program(flag, far):
    pg = engine.Program.__new__(engine.Program)
    pg.lib = L.load()
    pg.h2_flag = _FLAG if flag else None
    pg.far_plans = far
    return pg


def case(key, v, tuned_rows=None):
    """(program, args, keyword arguments of Program.plan) of one case; the images are registered as a side effect."""
    a = base_args(key) if tuned_rows is None else tuned_rows
    m = a.M
    a = type(a).from_buffer_copy(a)
    set_rows(a, {"tuned": m, "eighth": max(1, m // 8), "triple": 3 * m, "triple_eighth": 3 * m}[v["rows"]])
    if v["w_frag"]:
        a.w_frag = PTR
    if v["a_split"]:
        a.a_split, a.a_split_ld = PTR, (a.K + 7) // 8 * 8
    register_images(v["images"], a.N, a.K)
    kw = dict(scale_m=(8, 1) if v["rows"].endswith("eighth") else None, allow_splitk=v["allow_splitk"])
    if a.batch > 1:
        kw["batch_is_samples"] = v["alt_batch"]
    else:
        kw["per_sample"] = v["alt_batch"]
    return program(v["flag"], v["far"]), a, kw


def outcome(a):
    return tuple(int(bool(getattr(a, f))) if f in _AS_BOOL else int(getattr(a, f) or 0) for f in FIELDS)


def untouched(before, after):
    """True when every field of `after` outside FIELDS holds the bytes it held in `before`."""
    c = type(after).from_buffer_copy(after)
    for f in FIELDS:
        setattr(c, f, getattr(before, f))
    return bytes(c) == bytes(before)


def _check(lib, a, **trial):
    t = type(a).from_buffer_copy(a)
    for k, val in trial.items():
        setattr(t, k, val)
    return lib.ldmk_igemm_check(C.byref(t)) == 0


def classify(pg, before, kw, after):
    """The outcome classes this case belongs to, told from the inputs, the public table lookups and the library's own checks."""
    out = []
    scale = kw.get("scale_m")
    sample_batch = kw.get("per_sample", False) or (before.batch > 1 and kw.get("batch_is_samples", True))
    if sample_batch:
        if scale is not None and before.batch > 1:
            out.append("sample_batch_scales_batch")
        out.append("plain_heuristic")
        return out
    pm = before.M * scale[0] // scale[1] if scale is not None else before.M
    far, flag = pg.far_plans, pg.h2_flag is not None
    virt = dict(splitk_ws=1, splitk_ws_elems=1 << 40)
    eligible = before.compute == L.COMPUTE_F32 and not before.b_trans and not before.raw_slabs
    hp = engine.h2_plan(before, pm, far) if flag and eligible else None
    xp = engine.x3_plan(before, pm, far) if eligible else None
    fp = engine.tuned_plan(before, pm, far)
    if after.compute == L.COMPUTE_F16X2:
        if hp is not None:
            out.append("f16x2_from_its_section")
        elif xp is not None:
            if (xp[0], after.tile_cfg) in ((21, 5), (22, 1)):
                out.append("f16x2_via_x3_key_21_to_5" if xp[0] == 21 else "f16x2_via_x3_key_22_to_1")
        else:
            out.append("long_k_conv_rule_tuned_f32_plan" if fp is not None else "long_k_conv_rule_heuristic_plan")
        return out
    if after.compute == L.COMPUTE_BF16X3:
        if after.tile_cfg <= 6 and after.a_split:
            out.append("bf16x3_lds_tile_a_split_kept")
        if after.tile_cfg in (21, 22) and before.a_split and not after.a_split:
            out.append("bf16x3_ws_tile_a_split_dropped")
        return out
    p = hp if hp is not None else xp
    a_sp = bool(before.a_split) and p is not None and p[0] <= 6          # (the warp-specialised tiles drop a pre-split A)
    h2 = flag and ops.split_h2_of(before.w) is not None and not a_sp
    if p is not None and eligible and (h2 or ops.split_of(before.w) is not None):
        # a split plan with its images at hand that still ended in f32: refused for the policy problem alone?
        img = dict(compute=L.COMPUTE_BF16X3, w_split=PTR, w_split_ld=(before.K + 7) // 8 * 8, tile_cfg=p[0], splitk=p[1], **virt)
        if h2:
            img.update(compute=L.COMPUTE_F16X2, range_flag=PTR, w_scale_exp=SCALE_EXP, tile_cfg={21: 5, 22: 1}.get(p[0], p[0]))
        if not a_sp:
            img.update(a_split=0, a_split_ld=0)
        if _check(pg.lib, before, **img) and not _check(pg.lib, before, M=pm, **img):
            out.append("split_plan_legal_for_real_not_policy_problem")
    if fp is not None and fp[0] > 6:
        if after.tile_cfg == fp[0]:
            out.append("row_or_slab_tile_accepted")
        elif not before.w_frag:
            out.append("row_or_slab_tile_no_w_frag")
        else:
            trial = dict(tile_cfg=fp[0], splitk=1 if fp[0] <= 12 else fp[1], a_split=after.a_split, a_split_ld=after.a_split_ld, **virt)
            if _check(pg.lib, before, M=pm, **trial) and not _check(pg.lib, before, **trial):
                out.append("row_or_slab_tile_refused_for_real_problem")
    elif fp is None:
        out.append("plain_heuristic")
    return out


def shapes():
    """{rest of the key after M: its keys by rising M}."""
    out = {}
    for key in sorted(keys(), key=lambda k: int(k.split(",", 1)[0])):
        out.setdefault(key.split(",", 1)[1], []).append(key)
    return dict(sorted(out.items()))


def outcomes(key, classes=None):
    """Plan every variant of `key`: the list of outcomes.  Raises when a call changed a field outside FIELDS or returned something
    other than the (tile_cfg, splitk) it left in the args; classes: {class: [count, key, variant]} to tally into."""
    tuned_rows, out = base_args(key), []
    for i, v in enumerate(VARIANTS):
        pg, a, kw = case(key, v, tuned_rows)
        before = type(a).from_buffer_copy(a)
        ret = pg.plan(a, **kw)
        assert untouched(before, a) and tuple(ret) == (a.tile_cfg, a.splitk), (key, v, ret)
        out.append(outcome(a))
        for c in classify(pg, before, kw, a) if classes is not None else ():
            if classes[c][0] == 0:
                classes[c][1:] = [key, i]
            classes[c][0] += 1
    return out


def digest(shape_keys, classes=None):
    h = hashlib.sha256()
    for key in shape_keys:
        h.update(repr((key, outcomes(key, classes))).encode())
    return h.hexdigest()[:16]


def record():
    classes = {c: [0, None, None] for c in CLASSES}
    sh = {rest: digest(ks, classes) for rest, ks in shapes().items()}
    return dict(fields=list(FIELDS), variants=len(VARIANTS), cases=len(keys()) * len(VARIANTS), shapes=sh, classes=classes)


if __name__ == "__main__":
    if sys.argv[1:2] == ["--dump"]:
        for key in shapes()[sys.argv[2]]:
            for v, o in zip(VARIANTS, outcomes(key)):
                print(key, " ".join(f"{k}={x}" for k, x in v.items()), "->", " ".join(f"{f}={x}" for f, x in zip(FIELDS, o)))
        sys.exit(0)
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    rec = record()
    with open(path, "w") as fh:
        rows = lambda d: "{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in d.items()) + "\n}"      # one entry per line
        fh.write(rows({k: v for k, v in rec.items() if k not in ("shapes", "classes")})[:-2]
                 + f',\n"shapes": {rows(rec["shapes"])},\n"classes": {rows(rec["classes"])}\n}}\n')
    print(f"{rec['cases']} cases ({len(VARIANTS)} variants of each key), {len(rec['shapes'])} shapes -> {path}")
    for c, (n, key, i) in rec["classes"].items():
        print(f"{c:48s} {n:8d}  e.g. {key} variant {i}")
