"""CPU check of tests/kf_store_cases.py: the numpy restatement of a keyframe's grid CSR against the oracle's Frame grid -- the grid that
tests/test_gpu_grid.py holds ygzf_features_in_area to (oracle.features_in_area: Frame::AssignFeaturesToGrid + GetFeaturesInArea, pinned to the
reference's src/Frame.cc by tests/test_ref_frame.py) -- on the constructed key sets and on make_kf keyframes.

A window that covers every cell returns the cells' lists concatenated in the reference's order, columns then rows then key index: that IS the
CSR's list.  Smaller windows, answered from cell_start, hold the prefix to the same grid."""
import numpy as np
import pytest

from tests import kf_store_cases as K

ALL = dict(K.constructed_sets(), **K.seeded_keyframes())


def test_c_round_is_roundf():
    v = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 0.49999997, 0.50000006, -0.49999997, 63.5, 63.499996, 8388609.0, -0.0], np.float32)
    assert K.c_round(v).tolist() == [1, 2, 3, -1, -2, 0, 1, 0, 64, 63, 8388609, 0]


@pytest.mark.parametrize("name", sorted(ALL))
def test_csr_equals_oracle_grid(oracle, name):
    kf = ALL[name]
    keys, cam, sf, w, h = kf["keys"], kf["cam"], kf["scale_factors"], kf["w"], kf["h"]
    cs, lst = K.grid_csr(keys, cam)
    n = len(keys)
    total = int(cs[K.CELLS])
    assert cs[0] == 0 and (np.diff(cs) >= 0).all() and total <= n
    assert (lst[total:] == -1).all() and sorted(lst[:total].tolist()) == np.nonzero(K.pos_in_grid(keys, cam)[2])[0].tolist()
    whole = oracle.features_in_area(keys, sf, w, h, w / 2.0, h / 2.0, 4.0 * (w + h))
    assert np.array_equal(whole, lst[:total]), name
    rng = np.random.default_rng(len(name) + n)
    for _ in range(60):
        x, y = float(rng.uniform(-30, w + 30)), float(rng.uniform(-30, h + 30))
        r = float(rng.choice([0.5, 3.0, 9.0, 15.0, 40.0, 130.0]))
        exp = oracle.features_in_area(keys, sf, w, h, x, y, r)
        assert np.array_equal(K.features_in_area_csr(keys, cam, cs, lst, x, y, r), exp), (name, x, y, r)
    for i in rng.permutation(n)[:30]:                               # windows centred on keys: |dist| == 0 and the key's own cell
        x, y = float(keys["x"][i]), float(keys["y"][i])
        for r in (1.0, 12.0):
            exp = oracle.features_in_area(keys, sf, w, h, x, y, r)
            assert np.array_equal(K.features_in_area_csr(keys, cam, cs, lst, x, y, r), exp), (name, int(i), r)


def test_constructed_sets_are_what_they_claim():
    S = K.constructed_sets()
    # the half-cell keys: the product is exactly k + 0.5 for the middle one of each triple, and the three fall in (lower, upper, upper)
    kf = S["half_cells"]
    inv_w, inv_h = K.grid_inverses(kf["cam"])
    px, py, inside = K.pos_in_grid(kf["keys"], kf["cam"])
    vx = kf["keys"]["x"] * inv_w
    vy = kf["keys"]["y"] * inv_h
    halves = [i for i in range(len(vx)) if vx[i] - np.floor(vx[i]) == 0.5 or vy[i] - np.floor(vy[i]) == 0.5]
    assert len(halves) >= 4 and inside.all()
    for i in halves:                                                 # b sits between its two witnesses; its triple is 3 keys apart
        if vx[i] - np.floor(vx[i]) == 0.5:
            assert px[i - 3] == px[i] - 1 and px[i + 3] == px[i] and px[i] == int(np.floor(vx[i])) + 1
        else:
            assert py[i - 3] == py[i] - 1 and py[i + 3] == py[i] and py[i] == int(np.floor(vy[i])) + 1
    kf = S["last_column_row"]
    px, py, inside = K.pos_in_grid(kf["keys"], kf["cam"])
    assert inside.tolist() == [True, False, False, False, True, False, False, False, False, True, False, True, True, True]
    assert px[0] == 63 and px[1] == 64 and py[4] == 47 and py[5] == 48 and px[8] == -1 and py[10] == -1 and (px[13], py[13]) == (63, 47)
    kf = S["crowded_cell"]
    cs, _ = K.grid_csr(kf["keys"], kf["cam"])
    assert np.diff(cs).max() >= 300
    assert len(S["empty"]["keys"]) == 0 and len(S["one_key"]["keys"]) == 1
    assert [len(S["n_%d" % n]["keys"]) for n in (1023, 1024, 1025)] == [1023, 1024, 1025]
