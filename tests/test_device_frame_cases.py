"""The device-frame layouts of tests/device_frame_cases.py are what they claim to be (no GPU): the views cut back out of a buffer are the tight
frames, everything else is garbage with room for an aligned over-read on both sides, every case has the classes it is named for, and between them
the cases reach every branch the device entry point has to itself.  A class that no case reaches fails here, before a GPU is asked."""
import numpy as np
import pytest

from tests import device_frame_cases as D

LAYOUTS = D.all_layouts()


@pytest.mark.parametrize("case,lay", LAYOUTS, ids=[lay.name for _, lay in LAYOUTS])
def test_buffer_holds_the_frames_and_garbage(case, lay):
    frames = D.case_frames(case)
    buf, off0 = D.layout_buffer(lay, frames)
    args = (off0, lay.n, lay.h, lay.w, lay.row_pitch, lay.frame_stride)
    assert np.array_equal(D.frame_views(buf, *args), frames)
    mask = D.pixel_mask(buf.size, *args)
    assert mask.sum() == frames.size                                                  # no two pixels share a byte
    # every byte that is not a pixel is the seeded random stream, and that stream is garbage: spread like uniform bytes (sigma 73.9), no runs
    g = D.garbage(buf.size, 0x5EED)
    assert np.array_equal(buf[~mask], g[~mask])
    out = buf[~mask]
    assert out.std() > 65 and len(np.unique(out)) > 128 and (out[1:] == out[:-1]).mean() < 0.02
    other, off1 = D.layout_buffer(lay, frames, garbage_seed=77)
    assert off1 == off0 and np.array_equal(other[mask], buf[mask]) and (other[~mask] != buf[~mask]).mean() > 0.99
    # slack: row_pitch + 64 bytes in front of frame 0 and behind the last pixel, so that an aligned over-read stays inside the buffer
    first, last = np.flatnonzero(mask)[[0, -1]]
    assert first == off0 and first >= lay.row_pitch + 64 and buf.size - 1 - last >= lay.row_pitch + 64
    assert off0 + (lay.n - 1) * lay.frame_stride + lay.h * lay.row_pitch <= buf.size  # what pyr_tile bounds itself by
    assert (off0 - lay.base_offset) % D.BUFFER_ALIGN == 0
    # what ygzf_extract_batch_device accepts
    assert lay.row_pitch >= lay.w and lay.row_pitch % 4 == 0 and lay.frame_stride % 4 == 0 and lay.base_offset % 4 == 0


@pytest.mark.parametrize("case", D.CASES, ids=[c.name for c in D.CASES])
def test_case_has_the_classes_it_is_named_for(case):
    assert case.layouts and all((lay.w, lay.h) == (case.w, case.h) for lay in case.layouts)
    for lay in case.layouts:
        cl = D.layout_classes(lay)
        assert cl["wide_window"] and not cl["own_layout"]
        for key, want in case.expect.items():
            got = cl[key][0] if key == "base_mod16" else cl[key]
            assert got == want, (lay.name, key, got, want)
    if case.name == "offset_base":                          # consecutive frames fall into different mod-16 classes
        assert sorted(D.layout_classes(lay)["base_mod16"][0] for lay in case.layouts) == [4, 8, 12]
        assert all(len(set(D.layout_classes(lay)["base_mod16"])) == lay.n for lay in case.layouts)
    if case.name == "tight12":
        assert case.h % 2 == 1 and D.layout_classes(case.layouts[0])["stride_mod16"] != 0
    if case.name.startswith("oddwidth") or case.name == "crop":
        assert all(lay.row_pitch > lay.w for lay in case.layouts)
    if case.name == "crop":
        assert D.CROP_X0 % 4 == 0 and D.CROP_X0 % 16 != 0 and D.CROP_X0 + case.w <= D.CROP_IMAGE_W and D.CROP_Y0 + case.h <= D.CROP_IMAGE_H
    if case.name == "pitch_sequence":
        assert len({lay.row_pitch for lay in case.layouts}) == 3
    # several 30-pixel cells on level 0 and at least one on the last level
    lw, lh = D.level_size(case.w, case.h, case.nlevels - 1)
    assert (case.w - 29) // 30 >= 4 and (case.h - 29) // 30 >= 3 and (lw - 29) // 30 >= 1 and (lh - 29) // 30 >= 1


def test_cases_cover_every_class():
    reached = {"pitch_mod16": set(), "base_mod16": set(), "stride_mod16_nonzero": set(), "pyr_tail": set()}
    for case, lay in LAYOUTS + [(None, lay) for lay in D.STEREO_LAYOUTS]:
        cl = D.layout_classes(lay)
        reached["pitch_mod16"].add(cl["pitch_mod16"])
        reached["base_mod16"].update(cl["base_mod16"])
        reached["stride_mod16_nonzero"].add(cl["stride_mod16"] != 0)
        reached["pyr_tail"].add(cl["pyr_tail"])
        assert cl["wide_window"], lay.name
        # never the library's own layout.  The pitch is no multiple of 64 wherever the frames are the caller's whole allocation; a view into
        # larger images (the crop, the 1024-byte stereo rows) has the images' pitch and differs from the library's by its base or its pitch
        assert cl["pitch_mod64"] != 0 or (lay.row_pitch == 1024 and lay.row_pitch != D.align_up(lay.w, 64)), lay.name
        assert not cl["own_layout"], lay.name
    assert reached == {"pitch_mod16": {0, 4, 8, 12}, "base_mod16": {0, 4, 8, 12}, "stride_mod16_nonzero": {False, True}, "pyr_tail": {False, True}}


def test_tail_predicate_is_the_kernels_condition():
    """pyr_tail_reachable against the chunks written out by hand for three shapes (build_geometry's tile loop, csrc/ygzf_plan.hip; pyr_tile's
    `oo + 16 <= total`, csrc/extract_kernels.hip): 164 -> level 1 of 137 columns = a 128-column tile staging columns [0, 160) and a 32-column tile
    staging [152, 168): past a 164-byte last row, inside a 168-byte one."""
    cols, last_row = D.pyr_tile_chunks(164, 120)
    assert D.level_size(164, 120, 1) == (137, 100) and cols == [(0, 10), (152, 1)] and last_row == 119
    assert D.pyr_tail_reachable(164, 120, 164) and not D.pyr_tail_reachable(164, 120, 168) and not D.pyr_tail_reachable(164, 120, 1024)
    cols, last_row = D.pyr_tile_chunks(168, 120)
    assert cols == [(0, 10), (152, 1)] and last_row == 119 and not D.pyr_tail_reachable(168, 120, 168)
    cols, _ = D.pyr_tile_chunks(752, 480)                   # 627 columns: 256 + 256 + 128
    assert len(cols) == 3 and cols[0][0] == 0 and all(sxa % 4 == 0 and sxa + 16 * nc >= 752 or i < 2 for i, (sxa, nc) in enumerate(cols))


def test_describe_keys_stay_inside_the_reference_domain():
    for name in D.DESCRIBE_LAYOUTS:
        lay = next(lay for _, lay in LAYOUTS if lay.name == name)
        k = D.describe_keys(lay.w, lay.h)
        l0 = k[k["octave"] == 0]
        x, y = l0["x"].astype(int), l0["y"].astype(int)
        assert x.min() == 19 and x.max() == lay.w - 20 and y.min() == 19 and y.max() == lay.h - 20
        # every rowOff0: sixteen consecutive x on one row give sixteen consecutive window addresses
        base = D.layout_classes(lay)["base_mod16"][D.DESCRIBE_FRAME]
        for yy in (21, lay.h - 23):
            xs = x[(y == yy) & (x >= 21) & (x + 21 < lay.w)]
            assert {(base + (yy - 21) * lay.row_pitch + xx - 21) % 16 for xx in xs} == set(range(16))
        # both sides of every term of `interior`: kx >= 21, kx + 21 < gw, ky >= 21, ky + 22 < gh
        assert {20, 21} <= set(x) and {lay.w - 22, lay.w - 21} <= set(x) and {20, 21} <= set(y) and {lay.h - 23, lay.h - 22} <= set(y)
        assert set(np.unique(k["angle"])) == set(np.float32(D.DESCRIBE_ANGLES))
        l1 = k[k["octave"] == 1]
        w1, h1 = D.level_size(lay.w, lay.h, 1)
        lx, ly = np.rint(l1["x"] / np.float32(1.2)), np.rint(l1["y"] / np.float32(1.2))
        assert len(l1) >= 4 and lx.min() >= 19 and lx.max() <= w1 - 20 and ly.min() >= 19 and ly.max() <= h1 - 20


def test_stereo_scene_matches_on_octave_0(oracle):
    """only octave-0 matches make k_stereo_* read the caller's level 0: the chosen scene must give at least STEREO_MIN_OCTAVE0 of them"""
    pair = D.stereo_pair()
    oex = oracle.Extractor(D.STEREO_FEATURES, D.SCALE_FACTOR, D.STEREO_LEVELS, D.INI_TH, D.MIN_TH)
    kl, dl = oex.extract(pair[0])
    kr, dr = oex.extract(pair[1])
    ur, _ = oex.compute_stereo_matches(pair[0], pair[1], kl, dl, kr, dr, D.STEREO_MB, D.STEREO_MBF)
    assert int(((ur >= 0) & (kl["octave"] == 0)).sum()) >= D.STEREO_MIN_OCTAVE0
    for lay in D.STEREO_LAYOUTS:
        buf, off0 = D.layout_buffer(lay, pair)
        assert np.array_equal(D.frame_views(buf, off0, 2, lay.h, lay.w, lay.row_pitch, lay.frame_stride), pair)
