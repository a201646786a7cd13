"""One long-lived context across changing launches: a tracking thread keeps its context for a whole sequence and the multi-GPU entry points hand
a slot's context chunks of changing length (csrc/ygzf_mgpu.hip: the last chunk of a call is shorter).  Whatever a context keeps from one launch
to the next -- the octree's helper hand-over counters (keyed on the launch's layout), the plans chosen by frame count (k_pyr_strips up to
pyrStripFrames, the small octree plan up to 128 workgroups, the one-frame pyramid graph), the geometry and the carried previous frame -- must
give every call the bytes of the CPU oracle, whichever launch came before.  Every call is checked: keypoints (all fields), descriptors and the
matches of ygzf_match_batch_prev (pair 0 against the last frame the context extracted)."""
import os
import re

import numpy as np
import pytest

from tests.test_gpu_mgpu import _clip

pytestmark = pytest.mark.gpu

W, H, NF, NL, TH = 1920, 1080, 4000, 8, 15.0


class _env:
    """YGZF_FORCE / YGZF_DEBUG (csrc/ygzf_internal.h) while a context is created: both are read there"""
    def __init__(self, debug=None, **force):
        self.debug, self.force = debug, force

    def __enter__(self):
        from orb_ygz_slam_amd.capi import force_env
        self.old = {k: os.environ.get(k) for k in ("YGZF_FORCE", "YGZF_DEBUG")}
        os.environ["YGZF_FORCE"] = force_env(**self.force)
        if self.debug:
            os.environ["YGZF_DEBUG"] = self.debug
        else:
            os.environ.pop("YGZF_DEBUG", None)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class _Oracle:
    """the oracle's keypoints / descriptors per image and its SearchByProjection(Cur, Last) per (cur, last) pair, each computed once"""
    def __init__(self, oracle):
        from orb_ygz_slam_amd import EUROC
        self.O, self.cam = oracle, EUROC
        self.oex = oracle.Extractor(NF, 1.2, NL, 20, 7)
        self.sf = self.oex.tables()["scale"]
        self.kd, self.mt, self.pyr = {}, {}, {}

    def extract(self, key, img):
        if key not in self.kd:
            self.kd[key] = self.oex.extract(img)
        return self.kd[key]

    def pyramid(self, key, img):
        if key not in self.pyr:
            self.pyr[key] = self.oex.pyramid(img)
        return self.pyr[key]

    def match(self, cur, last, w, h):
        if (cur, last) not in self.mt:
            (k, d), (pk, pd) = self.kd[cur], self.kd[last]
            c = self.cam
            world = np.stack([(pk["x"] - np.float32(c["cx"])) / np.float32(c["fx"]), (pk["y"] - np.float32(c["cy"])) / np.float32(c["fy"]),
                              np.ones(len(pk), np.float32)], -1).astype(np.float32)
            I, z = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
            self.mt[(cur, last)] = self.O.search_by_projection_last(k, d, self.sf, w, h, c, pk, world, pd, I, z, I, z, TH, True, True, True)
        return self.mt[(cur, last)]


_IMGS = {}


def _images(w, h, n=4):
    """n distinct frames of one scene, a few pixels apart (tests/test_gpu_mgpu.py's clip): matches between any two of them"""
    if (w, h, n) not in _IMGS:
        _IMGS[(w, h, n)] = _clip(n, w, h)
    return _IMGS[(w, h, n)]


@pytest.fixture(scope="module")
def orc(oracle):
    return _Oracle(oracle)


def _check(ex, orc, keys, last, w, h, tag):
    """the context's last extraction held the frames `keys` (key = (w, h, index into _images)); pair 0 of the matcher must pair the first
    with `last` -- the key of the frame the context extracted before them, or None: an empty Last frame, no matches"""
    from orb_ygz_slam_amd import make_camera
    imgs = _images(w, h)
    ex.match_batch_prev(make_camera(w, h), TH, True, True, True)
    counts = ex.match_counts()
    assert len(counts) == len(keys)
    for f, key in enumerate(keys):
        k, d = ex.batch_fetch(f)
        ok, od = orc.extract(key, imgs[key[2]])
        assert len(k) == len(ok) and (k == ok).all() and (d == od).all(), (tag, f, "keypoints / descriptors")
        m, o = ex.match_fetch(f)
        prev = last if f == 0 else keys[f - 1]
        if prev is None:
            assert counts[f] == 0, (tag, f, "an empty Last frame")
            continue
        n, em, eo = orc.match(key, prev, w, h)
        assert counts[f] == n and (m[:len(k)] == em).all() and (o[:len(k)] == eo).all(), (tag, f, prev, "matches")


def _run(ex, orc, sizes, w=W, h=H, t0=0, last=None, after=None):
    """consecutive batches of the given sizes on ex; frame t of the stream is image t % 4.  -> (next t, key of the last frame)"""
    imgs = _images(w, h)
    t = t0
    for i, n in enumerate(sizes):
        keys = [(w, h, (t + j) % len(imgs)) for j in range(n)]
        ex.extract_batch_host(np.stack([imgs[k[2]] for k in keys]))
        _check(ex, orc, keys, last, w, h, (w, h, sizes, i))
        if after:
            after(n)
        t, last = t + n, keys[-1]
    return t, last


# launch sizes whose octree hand-over layout words = frames x levels x (helpers - 1) x bins collides on 256 CUs (6 / 8, 3 / 7, 2 / 14), and a walk
# across the small-octree limit (16 -> 17 frames of 8 levels) and pyrStripFrames in both directions, from and back to one-frame launches
SEQS = [[8, 6, 8, 8], [6, 8, 6], [3, 7, 3, 7], [2, 14, 2], [1, 4, 9, 16, 17, 20, 16, 9, 1]]


@pytest.mark.parametrize("seq", SEQS, ids=["-".join(map(str, s)) for s in SEQS])
def test_batch_size_sequences_on_one_context(orc, seq):
    """1920x1080 / 8 levels / 4000 features, the library's own plans: every call of the sequence equals the oracle"""
    from orb_ygz_slam_amd import Extractor
    with _env():
        ex = Extractor(NF, 1.2, NL, 20, 7, max_width=W, max_height=H, max_batch=20)
    _run(ex, orc, seq)
    ex.close()


_SMALL = re.compile(r"\[ygzf octree small plan: (\d+) frames, (\d+) workgroups per level; workgroups 0 that gave up waiting for their helpers, "
                    r"per level:([ \d]+); frames mask (0x[0-9a-f]+)\]")


@pytest.mark.parametrize("seq", SEQS, ids=["-".join(map(str, s)) for s in SEQS])
def test_no_workgroup_gives_up_on_its_helpers(orc, seq, capfd):
    """The same sequences on a context with YGZF_DEBUG=oct: k_octree counts the workgroups 0 that stopped waiting for their helper workgroups and
    computed a level alone, and the library prints the counts of every small-plan launch.  Nothing else runs on the device, so every helper starts
    at once: a give-up can only mean hand-over counters that lag the target the host passes (stale from an earlier launch of another layout)."""
    from orb_ygz_slam_amd import Extractor
    with _env(debug="oct"):
        ex = Extractor(NF, 1.2, NL, 20, 7, max_width=W, max_height=H, max_batch=20)
    capfd.readouterr()
    seen = []

    def after(n):
        lines = _SMALL.findall(capfd.readouterr().err)
        if n * NL <= 128:                                       # the small plan's launches (ygzf_ctx.h, octSmallWgs)
            assert len(lines) == 1, (seq, n, lines)
        for frames, helpers, per_level, mask in lines:
            assert int(frames) == n
            seen.append(int(helpers))
            gave_up = [int(v) for v in per_level.split()]
            assert len(gave_up) == NL
            assert sum(gave_up) == 0 and int(mask, 16) == 0, "workgroups 0 gave up on their helpers: %d frames, %d per (level, frame), per level %s, frames mask %s" % (
                n, int(helpers), gave_up, mask)
    _run(ex, orc, seq, after=after)
    ex.close()
    assert max(seen) > 1                                        # the sequence did take the helpers' plan (1920x1080 on a device of >= 128 CUs)


def test_image_size_switches_on_one_context(orc):
    """One context created for 1920x1080 takes 1920x1080 -> 752x480 -> 1280x720 -> 1920x1080 with changing batch sizes.  A new size rebuilds the
    geometry: the first match after it has an empty Last frame for pair 0 (include/ygzf.h), the next call carries again."""
    from orb_ygz_slam_amd import Extractor
    with _env():
        ex = Extractor(NF, 1.2, NL, 20, 7, max_width=W, max_height=H, max_batch=20)
    last = None
    for (w, h), sizes in (((W, H), [8, 3]), ((752, 480), [5, 1, 12]), ((1280, 720), [2, 9, 4]), ((W, H), [6, 8, 1])):
        _, last = _run(ex, orc, sizes, w, h, t0=1, last=None)   # (last=None: the size changed, nothing is carried into the first call)
    assert last is not None
    ex.close()


def _interleaved(orc, ahead=False):
    from orb_ygz_slam_amd import Extractor, make_camera, EUROC
    imgs = _images(W, H)
    with _env():
        ex = Extractor(NF, 1.2, NL, 20, 7, max_width=W, max_height=H, max_batch=20)
    ex.set_extract_ahead(ahead)
    key = lambda i: (W, H, i)
    last = None
    aligned = 0

    def one(i):
        k, d = ex.extract(imgs[i])
        ok, od = orc.extract(key(i), imgs[i])
        assert len(k) == len(ok) and (k == ok).all() and (d == od).all()

    def resident(i):
        ex.compute_pyramid(imgs[i])
        k, d = ex.extract_resident(W, H)
        ok, od = orc.extract(key(i), imgs[i])
        assert len(k) == len(ok) and (k == ok).all() and (d == od).all()

    def align_pair0(i, step):
        """pair 0 of ygzf_align_batch_prev: the carried frame `last` (keys at unit depth, its pyramid) against frame i -- extract-ahead saved the
        carried pyramid before frame i's overwrote it.  The first call only switches the pyramid carry on: no reference image yet."""
        nonlocal aligned
        ex.align_batch_prev(make_camera(W, H), NL - 1, 1, 10)
        ret, T, _ = ex.align_fetch(0)
        if not aligned:
            assert ret == 0, (step, ret)
        else:
            pk, _ = orc.extract(last, imgs[last[2]])
            world = np.stack([(pk["x"] - np.float32(EUROC["cx"])) / np.float32(EUROC["fx"]),
                              (pk["y"] - np.float32(EUROC["cy"])) / np.float32(EUROC["fy"]), np.ones(len(pk), np.float32)], -1).astype(np.float32)
            ident = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)
            o = orc.O.sparse_img_align(pk, world, ident, orc.pyramid(last, imgs[last[2]]), ident, orc.pyramid(key(i), imgs[i]),
                                       orc.oex.tables()["inv_scale"], EUROC, NL - 1, 1, device_order=True)
            assert ret == o[0] and ret > 100, (step, ret, o[0])
            assert np.abs(T - o[1]).max() <= 1e-5, (step, T, o[1])
        aligned += 1

    for step, (kind, idx) in enumerate([("one", [0]), ("batch", [1, 2, 3]), ("resident", [0]), ("one", [1]), ("resident", [2]),
                                        ("resident", [3]), ("batch", [0, 1]), ("resident", [2]), ("batch", [3, 0, 1, 2, 3])]):
        if kind == "one":
            one(idx[0])
        elif kind == "resident":
            resident(idx[0])
            if ahead:
                align_pair0(idx[0], step)
        else:
            ex.extract_batch_host(np.stack([imgs[i] for i in idx]))
        keys = [key(i) for i in idx]
        _check(ex, orc, keys, last, W, H, (step, kind))
        last = keys[-1]
    assert aligned == (4 if ahead else 0)
    ex.close()


def test_entry_points_interleaved(orc):
    """ygzf_extract (one frame), ygzf_extract_batch_host and ygzf_compute_pyramid + ygzf_extract_resident on one 1920x1080 context: after each,
    pair 0 of ygzf_match_batch_prev pairs the first frame with the last frame the context extracted -- whichever entry point extracted it."""
    _interleaved(orc)


def test_entry_points_interleaved_extract_ahead(orc):
    """The same with ygzf_set_extract_ahead: ygzf_compute_pyramid queues the extraction and ygzf_extract_resident collects it.  After every
    resident step pair 0 of ygzf_align_batch_prev aligns against the carried frame's pyramid, which compute_pyramid saved first."""
    _interleaved(orc, ahead=True)


def _make(max_batch=20):
    from orb_ygz_slam_amd import Extractor
    with _env():
        return Extractor(NF, 1.2, NL, 20, 7, max_width=W, max_height=H, max_batch=max_batch)


def _own_input_call(ex, orc, kind):
    imgs = _images(W, H)
    if kind == "dso":
        ex.extract_dso(imgs[0])
    elif kind == "dso_multilevel":
        ex.extract_dso_multilevel(imgs[0])
    elif kind == "fast_keypoint":
        ex.extract_fast_keypoint(imgs[0])
    else:
        (kl, dl), (kr, dr) = orc.extract((W, H, 0), imgs[0]), orc.extract((W, H, 1), imgs[1])
        ex.compute_stereo_matches(imgs[0], imgs[1], kl, dl, kr, dr, 0.11, 0.11 * 435.0)


OWN_INPUT = ["dso", "dso_multilevel", "fast_keypoint", "stereo_matches"]


@pytest.mark.parametrize("kind", OWN_INPUT)
def test_calls_that_take_the_buffers_end_the_batch(orc, kind):
    """ygzf_extract_dso (and its multi-level form), ygzf_extract_fast_keypoint and ygzf_compute_stereo_matches take the output buffers for their
    own inputs: no extracted batch afterwards, the next extraction carries nothing (pair 0 has an empty Last frame), the one after it carries again."""
    from orb_ygz_slam_amd import make_camera
    from orb_ygz_slam_amd.capi import YgzfError
    ex = _make()
    t, last = _run(ex, orc, [2])
    _own_input_call(ex, orc, kind)
    with pytest.raises(YgzfError):
        ex.match_batch_prev(make_camera(W, H), TH, True, True, True)
    _run(ex, orc, [2, 1], t0=t, last=None)
    ex.close()


def test_carry_switched_off_and_on(orc):
    """ygzf_set_carry_previous(0): an extraction returns the oracle's bytes, the batch matcher and aligner refuse; switched on again, the next
    extraction carries the then-last frame."""
    from orb_ygz_slam_amd import make_camera
    from orb_ygz_slam_amd.capi import YgzfError
    imgs = _images(W, H)
    ex = _make()
    t, _ = _run(ex, orc, [2])
    ex.set_carry_previous(False)
    for idx in ([2], [3, 0]):
        ex.extract_batch_host(np.stack([imgs[i] for i in idx]))
        for f, i in enumerate(idx):
            k, d = ex.batch_fetch(f)
            ok, od = orc.extract((W, H, i), imgs[i])
            assert len(k) == len(ok) and (k == ok).all() and (d == od).all()
        with pytest.raises(YgzfError):
            ex.match_batch_prev(make_camera(W, H), TH, True, True, True)
        with pytest.raises(YgzfError):
            ex.align_batch_prev(make_camera(W, H), NL - 1, 1, 10)
    ex.set_carry_previous(True)
    _run(ex, orc, [2, 3], t0=1, last=(W, H, 0))
    ex.close()


def test_has_resident_image_after_each_entry_point(orc):
    """ygzf_has_resident_image (include/ygzf.h): the context holds an image with its pyramid after ygzf_compute_pyramid, ygzf_extract and
    ygzf_extract_resident -- and after the batch extractions from host memory, whose frame 0 lies in the same buffers -- for that size only; not
    after a call that takes the buffers for its own inputs, nor on a new context."""
    imgs = _images(W, H)
    small = _images(752, 480)
    ex = _make()
    held = lambda: (ex.has_resident_image(W, H), ex.has_resident_image(752, 480))
    assert held() == (False, False)
    steps = [("extract", lambda: ex.extract(imgs[0]), (True, False)),
             ("extract_batch_host", lambda: ex.extract_batch_host(np.stack(imgs[1:3])), (True, False)),
             ("extract_dso", lambda: ex.extract_dso(imgs[0]), (False, False)),
             ("extract_batch_host_frames", lambda: ex.extract_batch_host_frames([imgs[3], imgs[0]]), (True, False)),
             ("compute_pyramid", lambda: ex.compute_pyramid(imgs[1]), (True, False)),
             ("extract_resident", lambda: ex.extract_resident(W, H), (True, False)),
             ("extract_fast_keypoint", lambda: ex.extract_fast_keypoint(imgs[2]), (False, False)),
             ("compute_pyramid", lambda: ex.compute_pyramid(imgs[2]), (True, False)),
             ("size change", lambda: ex.extract(small[0]), (False, True)),
             ("compute_stereo_matches", lambda: _own_input_call(ex, orc, "stereo_matches"), (False, False)),
             ("ahead on", lambda: ex.set_extract_ahead(True), (False, False)),
             ("compute_pyramid ahead", lambda: ex.compute_pyramid(imgs[3]), (True, False)),
             ("extract_resident ahead", lambda: ex.extract_resident(W, H), (True, False)),
             ("extract_dso", lambda: ex.extract_dso(imgs[0]), (False, False)),
             ("compute_pyramid ahead", lambda: ex.compute_pyramid(small[1]), (False, True))]
    for name, call, want in steps:
        call()
        assert held() == want, (name, held(), want)
    ex.close()


def _mgpu_check(orc, frames, got, unit, tag):
    k, d, c, m, nm = got
    for f in range(len(frames)):
        ok, od = orc.extract(("mgpu", f), frames[f])
        n = c[f]
        assert n == len(ok) and (k[f, :n] == ok).all() and (d[f, :n] == od).all(), (tag, f, "keypoints / descriptors")
        if f % unit == 0:
            assert nm[f] == -1, (tag, f)                        # the first frame of a unit has no predecessor
            continue
        en, em, _ = orc.match(("mgpu", f), ("mgpu", f - 1), frames.shape[2], frames.shape[1])
        assert nm[f] == en and (m[f, :n] == em).all(), (tag, f, "matches")


def test_mgpu_tail_chunks_on_one_slot(orc):
    """ygzf_mgpu_extract_match on one device slot with chunks of 8 frames.  Long units (unit = the call's frames): every chunk on context 0 of the
    slot -- 14 frames as 8 + 6, again, then 16 as 8 + 8.  Short units (unit 2 <= chunk): chunks alternate between the slot's two contexts -- 22
    frames as 8 / 8 / 6, context 0 takes 8 then 6."""
    from orb_ygz_slam_amd import MultiGpu, make_camera
    frames = _clip(22, W, H)
    cam = make_camera(W, H)
    with _env(mgpu_chunk=8):
        mg = MultiGpu([0], NF, 1.2, NL, 20, 7, max_width=W, max_height=H, max_frames_per_device=22)
    assert mg.chunk_frames() == 8
    for i, n in enumerate((14, 14, 16)):
        got = mg.extract_match(frames[:n], unit=n, cam=cam, th=TH)
        _mgpu_check(orc, frames[:n], got, n, ("long unit", i, n))
    for i in range(2):
        got = mg.extract_match(frames, unit=2, cam=cam, th=TH)
        _mgpu_check(orc, frames, got, 2, ("short units", i))
    mg.close()


_OCT_PLAN = re.compile(r"\[ygzf octree (small plan|histogram plan|sort plan|single launch)")


def test_plan_pins_outlive_a_geometry_change(oracle, capfd):
    """YGZF_FORCE is read when the context is created (csrc/ygzf_plan.h, PlanPins) and holds for every geometry the context meets afterwards: a
    context created with oct_plan=sort -- the environment restored right after, as every helper here does -- extracts two 320x240 frames, then two
    200x150 frames.  Launches of so few workgroups are the small histogram plan's unless the sort plan is pinned: both extractions must report
    the sort plan's launches and no small plan, and give the oracle's keypoints and descriptors."""
    from orb_ygz_slam_amd import Extractor
    nf, nl = 300, 3
    with _env(debug="oct", oct_plan="sort"):
        ex = Extractor(nf, 1.2, nl, 20, 7, max_width=320, max_height=240, max_batch=2)
    oex = oracle.Extractor(nf, 1.2, nl, 20, 7)
    for w, h in ((320, 240), (200, 150)):
        imgs = _images(w, h, n=2)
        capfd.readouterr()
        ex.extract_batch_host(np.stack(imgs))
        ran = _OCT_PLAN.findall(capfd.readouterr().err)
        assert ran and all(p in ("sort plan", "single launch") for p in ran), ((w, h), ran)
        for f in range(2):
            k, d = ex.batch_fetch(f)
            ok, od = oex.extract(imgs[f])
            assert len(k) == len(ok) and (k == ok).all() and (d == od).all(), ((w, h), f)
    ex.close()
