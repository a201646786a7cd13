"""GPU tier of the constructed matcher cases (tests/matcher_cases.py; tests/test_matcher_cases.py holds the oracle to the reference's own
code on every one of them and proves that each case is the crowding / tie / edge it claims): the device equals the oracle in count, every
assignment, ownership and updated prev_matched -- under the library's own plan, one workgroup per pair, three workgroups per pair, fixed
lanes, and for the cases that leave the fixpoint also under the one-wave pass alone -- and ygzf_match_path_stats says which path the DATA
took, with no serial plan forced.

A launch is only spread over several workgroups from 128 queries on, so match_split=1 / =3 differ from the default plan for slots_exhausted, chain_150,
the level cases and the sizes of 128 and more alone; the other cases run one workgroup per pair under every plan."""
import numpy as np
import pytest

from tests import matcher_cases as MC

pytestmark = pytest.mark.gpu

CASES = MC.cases()
PLANS = [None, "match_split=1", "match_split=3", "match_lanes=fixed", "match_serial=1"]


@pytest.fixture(scope="module")
def ctx():
    """plan -> context, one per plan for this file (YGZF_FORCE is read when a context is created), closed when the file is done"""
    from orb_ygz_slam_amd import Extractor
    from orb_ygz_slam_amd.capi import force_env
    made = {}

    def get(plan):
        if plan not in made:
            kv = dict(match_split=None, match_lanes=None, match_serial=None)
            if plan:
                kv.update([plan.split("=")])
            with pytest.MonkeyPatch.context() as mp:
                mp.setenv("YGZF_FORCE", force_env(**kv))
                made[plan] = Extractor(1000, 1.2, 8, 20, 7, max_width=MC.W, max_height=MC.H, max_batch=1)
        return made[plan]
    yield get
    for ex in made.values():
        ex.close()


def _delta(ex, before):
    after = ex.match_path_stats()
    return {k: after[k] - before[k] for k in after}


# (the one-wave pass alone: for the cases that reach it by themselves; tests/test_gpu_match.py forces it on natural frames)
RUNS = [(c, p) for p in PLANS for c in CASES if p != "match_serial=1" or c.limit]


@pytest.mark.parametrize("case,plan", RUNS, ids=["%s-%r" % (p or "default", c) for c, p in RUNS])
def test_device_equals_oracle(oracle, ctx, case, plan):
    ex = ctx(plan)
    exp = MC.run_oracle(oracle, case)
    got = MC.run_device(ex, case, exp)
    assert MC.same(got, exp, case) is None, MC.same(got, exp, case)
    assert (exp[0] == 0) == case.none


@pytest.mark.parametrize("case", [c for c in CASES if c.expect], ids=[repr(c) for c in CASES if c.expect])
def test_the_data_takes_the_path(oracle, ctx, case):
    """The counters of the rare paths, per case, under the library's own plan: extensions without hand-over, hand-over for lack of extension
    room, hand-over at the round cap, rescans of the one-wave pass -- and none of them where the case is not about them."""
    ex = ctx(None)
    exp = MC.run_oracle(oracle, case)
    before = ex.match_path_stats()
    got = MC.run_device(ex, case, exp)
    d = _delta(ex, before)
    assert MC.same(got, exp, case) is None
    print(repr(case), d)
    for key, want in case.expect.items():
        assert (d[key] > 0) if want == ">0" else (d[key] == want), (key, want, d)
    assert d["fallbacks"] == d["round_cap"] + d["ext_room"] and d["fallbacks"] <= 1
    assert ex.match_fallbacks() == ex.match_path_stats()["fallbacks"]


def test_limit_natural_limit_on_one_context(oracle, ctx):
    """A context fed a case that uses up the extension slots / the rounds, then keypoints out of the extractor, then the first case again:
    the same three answers as on their own (stale extension slots, claims or hand-over flags would show)."""
    from orb_ygz_slam_amd.synth import synth_frame
    ex = ctx(None)
    base = synth_frame(91, MC.W + 16, MC.H + 16)
    ka, da = ex.extract(base[8:8 + MC.H, 8:8 + MC.W])
    kb, db = ex.extract(base[10:10 + MC.H, 5:5 + MC.W])
    world = np.stack([(ka["x"] - np.float32(256)) / np.float32(256), (ka["y"] - np.float32(192)) / np.float32(256), np.ones(len(ka), np.float32)], -1).astype(np.float32)
    from orb_ygz_slam_amd import make_camera
    cam = make_camera(MC.W, MC.H, 256.0, 256.0, 256.0, 192.0)
    e_nat = oracle.search_by_projection_last(kb, db, MC.SF, MC.W, MC.H, MC.CAM, ka, world, da, MC.I3, MC.Z3, MC.I3, MC.Z3, 15.0)
    assert e_nat[0] > 100
    for case in [c for c in CASES if c.limit]:
        exp = MC.run_oracle(oracle, case)
        for step in range(2):
            got = MC.run_device(ex, case, exp)
            assert MC.same(got, exp, case) is None, (case, step)
            before = ex.match_path_stats()
            g = ex.search_by_projection_last(cam, kb, db, ka, world, da, MC.I3, MC.Z3, MC.I3, MC.Z3, 15.0, scale_factors=MC.SF)
            assert g[0] == e_nat[0] and (g[1] == e_nat[1]).all() and (g[2] == e_nat[2]).all(), (case, step)
            assert _delta(ex, before)["fallbacks"] == 0
