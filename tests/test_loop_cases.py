"""CPU tier: the numpy restatement of the loop-closing searches (tests/loop_cases.py) on its own -- the constructed points do what their labels
say and each mutation moves exactly its points; every seeded scene the GPU tier uses holds accepted and rejected pairs at every test and both
sides of every threshold."""
import numpy as np
import pytest

from orb_ygz_slam_amd import loop_scene
from tests import loop_cases as LC

SEEDS = (1, 2, 3)


def test_constructed_scw_points(oracle):
    for seed in (0, 1, 2):
        kf, pts, labels, km = LC.constructed_scw(oracle, seed)
        ri, rd = LC.ref_search(oracle, kf, *pts, 10.0, "proj", key_matched=km)
        assert dict(zip(labels, ri[:, 0] >= 0)) == LC.SCW_EXPECT
        for mutation, flips in LC.SCW_FLIPS.items():
            mi, _ = LC.ref_search(oracle, kf, *pts, 10.0, "proj", key_matched=km, mutation=mutation)
            assert {lab for lab, a, b in zip(labels, mi[:, 0], ri[:, 0]) if a != b} == flips, (seed, mutation)
        fi, _ = LC.ref_search(oracle, kf, *pts, 4.0, "fuse")
        for mutation in ("norm_float", "dot_float"):
            mi, _ = LC.ref_search(oracle, kf, *pts, 4.0, "fuse", mutation=mutation)
            assert {lab for lab, a, b in zip(labels, mi[:, 0], fi[:, 0]) if a != b} == LC.SCW_FLIPS[mutation], (seed, mutation)


def test_constructed_sim3_points(oracle):
    for seed in (0, 1, 2):
        kf, pts, labels, R2, t2 = LC.constructed_sim3(seed)
        ri, _ = LC.ref_search(oracle, kf, *pts, 7.5, "sim3", R2=R2, t2=t2)
        assert dict(zip(labels, ri[:, 0] >= 0)) == LC.SIM3_EXPECT
        mi, _ = LC.ref_search(oracle, kf, *pts, 7.5, "sim3", R2=R2, t2=t2, mutation="sim3_world_norm")
        assert dict(zip(labels, mi[:, 0] >= 0)) == {k: not v for k, v in LC.SIM3_EXPECT.items()}
        for mutation in ("norm_float", "dot_float", "no_key_matched"):
            mi, _ = LC.ref_search(oracle, kf, *pts, 7.5, "sim3", R2=R2, t2=t2, mutation=mutation)
            assert (mi == ri).all()


@pytest.mark.parametrize("seed", SEEDS)
def test_loop_scene_quality(oracle, seed):
    """Every rejection test of the Scw searches ends some points and passes others; matches fall on both sides of TH_LOW; clusters compete."""
    kfs, pts = loop_scene.loop_scene(seed)
    ended = set()
    dists = []
    for kf in kfs:
        trace = []
        ri, rd = LC.ref_search(oracle, kf, *pts, 4.0, "fuse", trace=trace)
        ended |= {w if isinstance(w, str) else w[0] for _, w in trace}
        dists.append(rd[ri >= 0])
    assert ended >= {"behind", "image", "distance", "view", "none", "found"}, ended
    d = np.concatenate(dists)
    assert (d <= LC.TH_LOW).sum() > 20 and (d > LC.TH_LOW).sum() > 5 and (d == LC.TH_LOW).any() and (d == LC.TH_LOW + 1).any()
    # SearchByProjection: several points name the same best key (the clusters)
    ci, cd = LC.ref_search(oracle, kfs[0], *pts, 10.0, "proj", n_best=4, max_dist=LC.TH_LOW)
    first = ci[:, 0][ci[:, 0] >= 0]
    assert len(first) - len(set(first.tolist())) >= 10
    assert (ci[:, 1] >= 0).any() and (ci[:, 3] < 0).any()


@pytest.mark.parametrize("seed", SEEDS)
def test_sim3_pair_quality(oracle, seed):
    """SearchBySim3's pair: mutual matches, one-sided matches the agreement loop rejects, distances on both sides of TH_HIGH."""
    kf1, kf2, p1, p2, has1, has2, T = loop_scene.sim3_pair(seed)
    nf, m12, m1, m2 = LC.ref_sim3(oracle, kf1, kf2, p1, p2, T, 7.5, LC.TH_HIGH, skip1=1 - has1, skip2=1 - has2)
    assert nf > 30
    assert ((m1 >= 0) & (m12 < 0)).sum() > 5                                 # one-sided
    row = dict(kf2, Rcw=T["R1w"], tcw=T["t1w"])
    trace = []
    bi, bd = LC.ref_search(oracle, row, p1[0], None, *p1[1:], 7.5, "sim3", skip=1 - has1, R2=T["sR21"], t2=T["t21"], trace=trace)
    found = bd[bi >= 0]
    assert (found <= LC.TH_HIGH).any() and (found > LC.TH_HIGH).any()
    ended = {w if isinstance(w, str) else w[0] for _, w in trace}
    assert ended >= {"skip", "image", "distance", "none", "found"}, ended
