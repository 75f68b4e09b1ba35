"""CPU: engine.Program.plan / engine.select_plan against the decisions recorded from the commit before select_plan existed
(tests/golden/plan_decisions.json, written by tools/record_plan_decisions.py on that commit): every key of the f32 / bf16x3 / f16x2
sections of the plan file x every planning input.  ldmk_igemm_check / ldmk_igemm_plan are host code, so no GPU is needed."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rec():
    from dsml_thesis_amd.build import build_lib
    build_lib(verbose=False)
    with open(os.path.join(ROOT, "tests", "golden", "plan_decisions.json")) as fh:
        return json.load(fh)


@pytest.fixture()
def R(monkeypatch):
    from dsml_thesis_amd import engine, ops
    from tools import record_plan_decisions as R
    for v in ("LDMK_SPLIT_BF16", "LDMK_F16X2", "LDMK_PS", "LDMK_NO_PLAN_TABLE", *engine._SECTIONS.values()):
        monkeypatch.delenv(v, raising=False)
    engine.reset_tables()
    yield R
    ops._IMAGES.clear()
    engine.reset_tables()


def test_the_record_covers_the_whole_grid(rec, R):
    """Every key of the three sections, every variant, and at least one case in every outcome class the plan file can reach."""
    assert rec["fields"] == list(R.FIELDS) and rec["variants"] == len(R.VARIANTS) == 588
    assert sorted(rec["shapes"]) == sorted(R.shapes()) and len(R.keys()) > 900
    assert rec["cases"] == len(R.keys()) * len(R.VARIANTS)
    assert set(rec["classes"]) == set(R.CLASSES)
    assert {c for c, (n, _, _) in rec["classes"].items() if n == 0} == set(R.UNREACHABLE)


def test_plan_decides_what_the_recorded_commit_decided(rec, R):
    """Program.plan leaves in the args exactly what it left there before it was rebuilt on select_plan -- M, batch, tile_cfg, splitk,
    the scratch fields, compute, the weight-image fields, the range flag, a_split, raw_slabs -- returns (tile_cfg, splitk), and
    touches no other field of the struct (R.outcomes asserts the last two).  Compared per shape through the digest of all its
    outcomes; `python tools/record_plan_decisions.py --dump SHAPE` on both commits shows the cases behind a digest that differs."""
    bad = [rest for rest, ks in R.shapes().items() if R.digest(ks) != rec["shapes"][rest]]
    assert not bad, bad


def test_select_plan_leaves_its_args_alone(rec, R):
    """select_plan is a function of its inputs: on one case of every outcome class it returns the decision Program.plan applies and
    does not change a byte of the args."""
    from dsml_thesis_amd import engine, ops
    for c, (n, key, i) in rec["classes"].items():
        if n == 0:
            continue
        pg, a, kw = R.case(key, R.VARIANTS[i])
        before = bytes(a)
        images = engine.WeightImages(ops.split_of(a.w), ops.split_h2_of(a.w), bool(a.w_frag), bool(a.a_split))
        d = engine.select_plan(pg.lib, a, engine.PlanPolicy(pg.h2_flag, pg.far_plans), images, **kw)
        assert bytes(a) == before, c
        assert pg.plan(a, **kw) == (d.tile_cfg, d.splitk) and a.compute == d.compute and bool(a.a_split) == d.a_split, c
        assert bool(a.w_split) == (d.image is not None), c
