"""The octree's sort plan launches its levels in groups of their own workgroup size and LDS (csrc/ygzf_api.hip, plan_oct_sort; k_octree<.., kBlock>),
with the candidates' second sort buffer over the node arrays.  Same bytes as ONE launch of all levels (YGZF_FORCE=oct_groups=1) and as the oracle:
on the bench geometries, on odd geometries and feature budgets, with every workgroup size forced, and with candidate budgets so small that levels
sort through global memory.

These launches carry a few frames, which the library would hand to the small histogram plan (ygzf_ctx.h, octSmallWgs): every context here pins
the sort plan (oct_plan=sort) and runs with YGZF_DEBUG=oct, and every test checks from the library's own report which launches actually ran --
their workgroup sizes, their candidate budgets and, where a test wants it, a level of frame 0 whose candidates did not fit that budget."""
import os
import re

import numpy as np
import pytest

from orb_ygz_slam_amd.synth import synth_frame
from tests.test_gpu_extract import _cmp_frame

pytestmark = pytest.mark.gpu

CASES = [
    # (w, h, nlevels, nfeatures, image)
    (752, 480, 8, 1000, lambda: synth_frame(51, 752, 480)),       # the default bench geometry: levels 0-3 and 4-7
    (640, 480, 8, 1000, lambda: synth_frame(52, 640, 480)),       # configs[1]
    (333, 517, 8, 1500, lambda: synth_frame(53, 333, 517)),       # tall: 1024 and 512 threads
    (1280, 360, 6, 1200, lambda: synth_frame(54, 1280, 360)),     # wide: four roots
    (701, 455, 7, 777, lambda: np.random.default_rng(5).integers(0, 256, (455, 701), dtype=np.uint8)),   # noise: more candidates than the budgets
]

_PLAN = re.compile(r"\[ygzf octree sort plan: (\d+) launches;(.*)\]")
_GROUP = re.compile(r"levels (\d+)-(\d+) threads (\d+) cap (\d+) candidates (\d+) lds (\d+);")
_LEVEL = re.compile(r"\[ygzf octree lvl (\d+), 10ns ticks\].* M=(\d+) n=(\d+)")
_OTHER = re.compile(r"\[ygzf octree (small|histogram) plan")


class _env:
    """YGZF_FORCE (the sort plan pinned, plus the given keys; None removes one) and YGZF_DEBUG=oct while a context is created"""
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        from orb_ygz_slam_amd.capi import force_env
        self.old = {k: os.environ.get(k) for k in ("YGZF_FORCE", "YGZF_DEBUG")}
        os.environ["YGZF_FORCE"] = force_env(base="", oct_plan="sort", **self.kv)
        os.environ["YGZF_DEBUG"] = "oct"

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _report(err, nlevels):
    """the sort plan's launches (l0, l1, threads, candidates) and frame 0's candidates per level, from one extraction's YGZF_DEBUG=oct lines"""
    assert not _OTHER.search(err), "another octree plan ran"
    plans = _PLAN.findall(err)
    assert len(plans) == 1, "the sort plan's launches did not run (exactly once)"
    groups = [(int(a), int(b), int(t), int(k)) for a, b, t, _, k, _ in _GROUP.findall(plans[0][1])]
    assert len(groups) == int(plans[0][0])
    assert [g[0] for g in groups] == [0] + [g[1] + 1 for g in groups[:-1]] and groups[-1][1] == nlevels - 1
    M = {int(l): int(m) for l, m, _ in _LEVEL.findall(err)}
    assert sorted(M) == list(range(nlevels))
    return groups, M


def _spilled(groups, M):
    return [l for a, b, _, k in groups for l in range(a, b + 1) if M[l] > k]


def _run(capfd, case, **force):
    from orb_ygz_slam_amd import Extractor
    w, h, nl, nf, make = CASES[case]
    img = make()
    imgs = np.stack([img, np.ascontiguousarray(img[::-1]), np.ascontiguousarray(img[:, ::-1])])
    with _env(**force):
        ex = Extractor(nf, 1.2, nl, 20, 7, max_width=w, max_height=h, max_batch=8)
    capfd.readouterr()
    ex.extract_batch_host(np.concatenate([imgs, imgs, imgs[:2]]))   # 8 frames: the launch sorts its describe order as the bench's do
    groups, M = _report(capfd.readouterr().err, nl)
    res = [ex.batch_fetch(f) for f in range(3)]
    return ex, imgs, res, groups, M


@pytest.mark.parametrize("case", range(len(CASES)))
def test_grouped_plan_equals_one_launch_and_the_oracle(oracle, capfd, case):
    from orb_ygz_slam_amd.capi import octree_sort_plan_host
    w, h, nl, nf, _ = CASES[case]
    oex = oracle.Extractor(nf, 1.2, nl, 20, 7)
    ex, imgs, grouped, groups, _ = _run(capfd, case, oct_groups=None)
    plan = octree_sort_plan_host(nf, 1.2, nl, w, h)
    assert groups == [(g["l0"], g["l0"] + g["n"] - 1, g["block"], g["lds_cand"]) for g in plan]   # the launches that ran are the host plan's
    assert len(groups) >= 2
    for f in range(3):
        _cmp_frame(oracle, ex, oex, imgs[f], frame=f)
    ex.close()
    ex1, _, one, groups1, _ = _run(capfd, case, oct_groups=1)
    ex1.close()
    assert len(groups1) == 1 and groups1[0][2] == 1024
    for (k0, d0), (k1, d1) in zip(grouped, one):
        assert np.array_equal(k0, k1) and np.array_equal(d0, d1)


@pytest.mark.parametrize("case", [0, 2, 4])
@pytest.mark.parametrize("block,lds_kb,spill", [(256, None, False), (512, None, False), (1024, None, False), (256, 8, True), (512, 24, True),
                                                 (1024, 20, True)])
def test_every_workgroup_size_and_a_spilling_budget(oracle, capfd, case, block, lds_kb, spill):
    """block pins every launch's workgroup (256 threads on levels whose lists hold more than 256 nodes included); lds_kb a budget that leaves some
    or all of a level's candidates to the global sort buffers"""
    w, h, nl, nf, _ = CASES[case]
    oex = oracle.Extractor(nf, 1.2, nl, 20, 7)
    ex, imgs, _, groups, M = _run(capfd, case, oct_block=block, oct_lds_kb=lds_kb)
    assert all(t == block for _, _, t, _ in groups)
    if spill:
        assert _spilled(groups, M), "no level of frame 0 sorted through global memory"
    for f in range(3):
        _cmp_frame(oracle, ex, oex, imgs[f], frame=f)
    ex.close()


def test_the_bench_geometry_sorts_in_lds(capfd):
    """752x480 / 8 / 1000 on a frame of the synthetic clip: every level's candidates fit its launch's budget (no global sort in the default plan)"""
    ex, _, _, groups, M = _run(capfd, 0)
    ex.close()
    assert [(a, b, t) for a, b, t, _ in groups] == [(0, 3, 512), (4, 7, 256)]
    assert not _spilled(groups, M)


@pytest.mark.parametrize("seed", range(4))
def test_fuzzed_geometries(oracle, capfd, seed):
    from orb_ygz_slam_amd import Extractor
    rng = np.random.default_rng(900 + seed)
    w, h = int(rng.integers(200, 900)), int(rng.integers(160, 600))
    nl, nf = int(rng.integers(3, 9)), int(rng.integers(150, 2500))
    img = synth_frame(300 + seed, w, h)
    oex = oracle.Extractor(nf, 1.2, nl, 20, 7)
    outs, plans = [], []
    for groups in (None, 1):
        with _env(oct_groups=groups):
            ex = Extractor(nf, 1.2, nl, 20, 7, max_width=w, max_height=h, max_batch=6)
        capfd.readouterr()
        ex.extract_batch_host(np.stack([img] * 6))
        plans.append(_report(capfd.readouterr().err, nl)[0])
        _cmp_frame(oracle, ex, oex, img, frame=5)
        outs.append(ex.batch_fetch(5))
        ex.close()
    assert len(plans[1]) == 1
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
