"""Constructed inputs for MapPoint::ComputeDistinctiveDescriptors (k_distinctive for 1..256 observations, k_distinctive_large beyond), numpy only.

restate() follows src/MapPoint.cc:240-265 line for line: the full N x N Hamming matrix with a zero diagonal, every row sorted, the element at
(int)(0.5*(N-1)), the first minimum wins, -1 for a point without observations.  `form` swaps in ONE mistake a kernel could make (FORMS); every
case lists in `wrong` the forms that must change its answer, and tests/test_distinctive_cases.py demands that exactly those do.

Descriptors are built to exact distances: thermo((x, y)) sets the first x of bits 0..127 and the first y of bits 128..255 (0 <= x, y <= 128), so
the Hamming distance of two observations is |dx| + |dy| and a median is plane geometry.  Almost every point here is two clusters far apart,
a `near` one that holds index k of every sorted row of its members and a `far` one whose rows read a cross distance there:

    near = one centre + a ring at distance r on both sides  ->  the centre's median is r, a ring member's is 2r: the centre wins alone
    far  = members 10 apart (or a centre and a ring, r = 5)

What cannot be decided: a form that loses or clamps the distance 256 (a 256-bin histogram, a bisection that stops at 255).  A row's median is
256 only if more than half of the observations are the bitwise complement of that row's; those are then identical to each other and have
median 0, so a median of 256 never wins and never ties the winner, and the entries below the median keep their places.  Distances 0 and 256
do occur in the rows (`complement_*`).  N = 2 cannot tell the two medians apart either: index 0 gives 0 in both rows and index 1 the same
distance in both, so the first row wins under both; that case pins the first of equal medians instead.  N = 3 and N = 4 read the
nearest-neighbour distance, which the two nearest share: their correct answer is always a tie, so "last_minimum" moves them too.
"""
import numpy as np

FORMS = ("upper_median",          # index N // 2
         "last_minimum",          # <= in place of <
         "padding_counts",        # the row is padded to a multiple of 64 with all-zero descriptors that are counted (a missing j < N mask)
         "tail_dropped",          # observations from 64 * (N // 64) on are ignored in the rows, N >= 64 (a loop over whole 64-steps only)
         "large_as_small",        # a point with N > 256 is treated as its first 256 observations
         "large_list_shifted",    # the large points' results are written to the batch slot one lower (the list read one entry early)
         "index_one_low")         # index k - 1: `count >= k` in place of `count > k` in the ballot bisection or in the histogram's running sum

UNWRITTEN = -2                    # what "large_list_shifted" leaves in a slot nobody wrote


def thermo(points):
    """(n, 2) integer points, 0 <= x, y <= 128 -> (n, 32) descriptors with Hamming distance |dx| + |dy|"""
    p = np.asarray(points, np.int64).reshape(-1, 2)
    assert ((p >= 0) & (p <= 128)).all()
    bits = np.concatenate([np.arange(128)[None, :] < p[:, :1], np.arange(128)[None, :] < p[:, 1:]], axis=1)
    return np.packbits(bits, axis=1)


def hamming_matrix(d):
    bits = np.unpackbits(np.ascontiguousarray(d, np.uint8), axis=1).astype(np.float32)      # counts <= 256: exact in float32
    s = bits.sum(1)
    D = (s[:, None] + s[None, :] - 2.0 * (bits @ bits.T)).astype(np.int64)
    np.fill_diagonal(D, 0)
    return D


def _point(d, form, info):
    N = len(d)
    if N == 0:
        return -1
    if form == "large_as_small" and N > 256:
        d, N = d[:256], 256
    D = hamming_matrix(d)                                                # Distances[i][j], Distances[i][i] = 0
    k = int(0.5 * (N - 1))
    if form == "upper_median":
        k = N // 2
    if form == "index_one_low":
        k = max(k - 1, 0)
    rows = D
    if form == "padding_counts" and N % 64:
        to_zero = np.unpackbits(d, axis=1).sum(1).astype(np.int64)
        rows = np.concatenate([D, np.repeat(to_zero[:, None], 64 - N % 64, axis=1)], axis=1)
    if form == "tail_dropped" and N >= 64:
        rows = D[:, :64 * (N // 64)]
    medians = np.sort(rows, axis=1)[:, k]                                # sort(vDists); median = vDists[0.5 * (N - 1)]
    if form == "last_minimum":
        best = N - 1 - int(np.argmin(medians[::-1]))
    else:
        best = int(np.argmin(medians))                                   # median < BestMedian: the first minimum
    if info is not None:
        info.update(N=N, k=k, medians=medians, upper=np.sort(D, axis=1)[:, N // 2], D=D)
    return best


def restate(obs_off, desc, form=None, trace=None):
    """-> winning observation index per point (int32).  trace: a list that receives one dict per point (N, k, medians, upper, D; {} if empty)."""
    assert form is None or form in FORMS, form
    off = np.asarray(obs_off, np.int64)
    d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    n = len(off) - 1
    out = np.zeros(n, np.int32)
    large = []
    for p in range(n):
        info = {}
        out[p] = _point(d[off[p]:off[p + 1]], form, info)
        if trace is not None:
            trace.append(info)
        if off[p + 1] - off[p] > 256:
            large.append(p)
    if form == "large_list_shifted":
        res = out[large].copy()
        out[large] = UNWRITTEN
        for p, r in zip(large, res):
            if p > 0:
                out[p - 1] = r
    return out


# ---- constructions ------------------------------------------------------------------------------------------------------------------------------
def ring(n, centre, r=2):
    """n points at distance r from (centre, 0) on the x axis, alternating below / above"""
    return [(centre - r, 0) if i % 2 == 0 else (centre + r, 0) for i in range(n)]


def two_clusters(N):
    """near = (20, 0) + a ring of radius 2, k + 1 members (k = (int)(0.5*(N-1))); far = the rest, alternating x = 100 / 110.  The near centre's
    median is 2 and nobody else's is below 4 (N >= 6).  At index N // 2 an even N reads the nearest cross distance instead, which the near
    ring's upper side (x = 22) and the far x = 100 share at 78 while the centre has 80.  The far cluster comes FIRST, the centre sits in
    the middle of the near one."""
    k = int(0.5 * (N - 1))
    near = ring(k, 20)
    near.insert(len(near) // 2, (20, 0))
    far = [(100, 0) if i % 2 == 0 else (110, 0) for i in range(N - k - 1)]
    return thermo(far + near), len(far) + near.index((20, 0))


def tail_point(N):
    """N = 64 q + 1.  (N - 1) / 2 observations at the origin come first, then (N + 1) / 2 far ones: a centre at x = 100 and a ring of radius 2,
    the LAST observation a ring member.  Right: the far cluster holds index k, its centre wins with 2.  With the last observation dropped
    the far rows read a cross distance (>= 98) at k as the origin rows do; with 63 zero descriptors counted the origin rows read 0."""
    assert N % 64 == 1
    m = (N - 1) // 2
    far = ring(m + 1, 100)
    far[m // 2] = (100, 0)
    return thermo([(0, 0)] * m + far), m + m // 2


def tie_point(N, i1, i2):
    """Two DIFFERENT descriptors with the same least median: (20, 63) and (20, 65) are 2 apart and 3 from every member of the ring (18, 64) /
    (22, 64), whose own medians are 4.  They go to rows i1 < i2; the rest of the near cluster (k + 1 members in all) and the far cluster
    (x = 100 / 110, y = 0) fill the other rows in order."""
    k = int(0.5 * (N - 1))
    near = [(18, 64) if i % 2 == 0 else (22, 64) for i in range(k - 1)]
    far = [(100, 0) if i % 2 == 0 else (110, 0) for i in range(N - k - 1)]
    rest = near + far
    pts = []
    for i in range(N):
        pts.append((20, 63) if i == i1 else (20, 65) if i == i2 else rest.pop(0))
    return thermo(pts)


def one_low_point(N):
    """N odd.  Near = ring members at x = 18 (k - 1 of them, first), ONE at x = 22, the centre x = 20 last; far behind.  The centre's median is 2,
    an x = 18 member reads 4 at index k (the one at x = 22) but 2 at index k - 1 (the centre): one index low, the first row ties and wins."""
    assert N % 2 == 1 and N >= 7
    k = (N - 1) // 2
    near = [(18, 0)] * (k - 1) + [(22, 0), (20, 0)]
    far = [(100, 0) if i % 2 == 0 else (110, 0) for i in range(N - k - 1)]
    return thermo(near + far), k


def spread_point(N):
    """N = 4 t + 1: t copies of each corner (0, 0), (128, 0), (0, 128), (128, 128) in turn and (60, 64) LAST.  Every corner row reads 128 at index
    k = 2 t (t zeros, one 124 or 132, 2 t entries at 128, t at 256); the last row reads 124 (2 t entries at 124, 2 t at 132) and wins alone: a
    least median far from 0, found among rows that hold 0, 128 and 256."""
    assert N % 4 == 1
    corners = [(0, 0), (128, 0), (0, 128), (128, 128)]
    return thermo([corners[i % 4] for i in range(N - 1)] + [(60, 64)]), N - 1


def handover_pair():
    """256 observations: near centre (20, 0) + 127 ring (r = 2), far centre (105, 0) + 127 ring (r = 5): k = 127, both clusters hold index k, the
    near centre wins 2 against 5.  The 257th observation is one more far ring member: k = 128 is now a cross distance for every near row and
    the far centre wins with 5."""
    near = ring(127, 20)
    near.insert(40, (20, 0))
    far = ring(127, 105, 5)
    far.insert(77, (105, 0))
    p256 = near + far
    return thermo(p256), thermo(p256 + [(110, 0)]), 40, 128 + 77


class Case:
    def __init__(self, name, points, reach, wrong):
        """points: one (n_i, 32) descriptor array per MapPoint of the batch"""
        self.name = name
        self.counts = [len(p) for p in points]
        self.off = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int32)
        self.desc = np.concatenate([np.asarray(p, np.uint8).reshape(-1, 32) for p in points] + [np.zeros((0, 32), np.uint8)])
        self.reach = reach                                               # (answer, trace) -> bool
        self.wrong = tuple(wrong)
        assert set(self.wrong) <= set(FORMS)

    def __repr__(self):
        return self.name

    @property
    def total(self):
        return int(self.off[-1])


def _unique_min(m, i):
    return int(np.argmin(m)) == i and int((m == m.min()).sum()) == 1


def cases():
    out = []
    add = lambda *a: out.append(Case(*a))
    LARGE = ("large_as_small", "large_list_shifted")

    # ---- the median index: even N in every register class and in the histogram kernel, the odd N beside each -----------------------------
    add("even_2", [thermo([(0, 0), (128, 128)])],
        lambda a, t: a[0] == 0 and t[0]["medians"].tolist() == [0, 0] and t[0]["upper"].tolist() == [256, 256], ["last_minimum"])
    add("even_4", [thermo([(0, 0), (1, 0), (10, 0), (12, 0)])],
        lambda a, t: a[0] == 0 and t[0]["medians"].tolist() == [1, 1, 2, 2] and int(np.argmin(t[0]["upper"])) == 1, ["upper_median", "last_minimum"])
    add("odd_3", [thermo([(20, 0), (22, 0), (100, 0)])],
        lambda a, t: a[0] == 0 and t[0]["medians"].tolist() == [2, 2, 78], ["last_minimum"])
    for N in (64, 128, 192, 256, 258, 320):
        d, c = two_clusters(N)
        add("even_%d" % N, [d], lambda a, t, c=c, N=N: a[0] == c and t[0]["k"] == N // 2 - 1 and _unique_min(t[0]["medians"], c) and
            t[0]["medians"][c] == 2 and int(np.argmin(t[0]["upper"])) != c and t[0]["upper"].min() == 78 and t[0]["upper"][c] == 80,
            ["upper_median"] + (list(LARGE) if N > 256 else []) + (["tail_dropped"] if N == 258 else []))
    for N in (63, 65, 129, 193, 255, 257, 321):
        d, c = two_clusters(N)
        add("odd_%d" % N, [d], lambda a, t, c=c, N=N: a[0] == c and t[0]["k"] == N // 2 == (N - 1) // 2 and _unique_min(t[0]["medians"], c),
            {257: ["large_list_shifted"], 321: list(LARGE)}.get(N, []) + ([] if N == 63 else ["tail_dropped"]))     # 63 < 64: no whole step to keep

    # ---- equal medians: the first one wins ---------------------------------------------------------------------------------------------------
    def tie_reach(i1, i2):
        return lambda a, t: (a[0] == i1 and t[0]["medians"][i1] == t[0]["medians"][i2] == 3 == t[0]["medians"].min() and
                             int((t[0]["medians"] == 3).sum()) == 2 and t[0]["D"][i1, i2] == 2)
    # (an even N reads a cross distance at N // 2, so "upper_median" moves those as well; the first 256 rows of the 300 and of the 320 hold the
    # first of the pair and still more than half of the near cluster, so "large_as_small" keeps their answer)
    U, S = "upper_median", "large_list_shifted"
    for N, i1, i2, extra in ((7, 0, 6, []), (64, 0, 63, [U]), (130, 5, 70, [U]), (256, 63, 192, [U]), (300, 0, 299, [U, S, "tail_dropped"]),
                             (320, 5, 300, [U, S]), (700, 100, 613, [U] + list(LARGE))):
        add("tie_%d_rows_%d_%d" % (N, i1, i2), [tie_point(N, i1, i2)], tie_reach(i1, i2), ["last_minimum"] + extra)
    for N in (7, 64, 300):
        add("identical_%d" % N, [np.repeat(thermo([(77, 31)]), N, axis=0)], lambda a, t: a[0] == 0 and not t[0]["D"].any(),
            ["last_minimum"] + (["large_list_shifted"] if N > 256 else []))
    add("complement_3", [thermo([(0, 0), (128, 128), (128, 128)])],
        lambda a, t: a[0] == 1 and t[0]["medians"].tolist() == [256, 0, 0] and t[0]["D"].max() == 256, ["last_minimum", "padding_counts", "index_one_low"])

    # ---- the last partial 64-step decides -----------------------------------------------------------------------------------------------------------
    for N in (65, 129, 193, 257, 321):
        d, c = tail_point(N)
        add("tail_%d" % N, [d], lambda a, t, c=c: a[0] == c and _unique_min(t[0]["medians"], c) and t[0]["medians"][c] == 2 and
            np.sort(t[0]["D"][:, :-1], axis=1)[:, t[0]["k"]].min() >= 98,
            ["padding_counts", "tail_dropped", "index_one_low"] + (list(LARGE) if N > 256 else []))     # (one index low, the origin rows read 0)

    # ---- a least median of 124 among rows that hold 0, 128 and 256 -----------------------------------------------------------------------------------
    for N in (5, 65, 257, 321):
        d, c = spread_point(N)
        add("spread_%d" % N, [d], lambda a, t, c=c: a[0] == c and _unique_min(t[0]["medians"], c) and t[0]["medians"][c] == 124 and
            (t[0]["medians"][:c] == 128).all() and set(np.unique(t[0]["D"][0]).tolist()) == {0, 124, 128, 256},
            # zero descriptors are copies of the first corner, whose row then reads 0 (not at 257 and 321: t + 63 zeros do not reach k); without
            # its own 0 the last row reads 132; one index low the first row of the 5 reads its 124
            {5: ["padding_counts", "index_one_low"], 65: ["padding_counts", "tail_dropped"]}.get(N, ["tail_dropped"] + list(LARGE)))

    # ---- one index low ----------------------------------------------------------------------------------------------------------------------------------
    for N in (7, 65, 257, 259):
        d, c = one_low_point(N)
        add("one_low_%d" % N, [d], lambda a, t, c=c: a[0] == c and _unique_min(t[0]["medians"], c) and
            np.sort(t[0]["D"], axis=1)[0, t[0]["k"] - 1] == 2, ["index_one_low"] + (list(LARGE) if N > 256 else []))

    # ---- the hand-over between the two kernels ----------------------------------------------------------------------------------------------------
    d256, d257, c256, c257 = handover_pair()
    add("handover_256_257", [d256, d257], lambda a, t: a.tolist() == [c256, c257] and (d257[:256] == d256).all() and _unique_min(t[0]["medians"], c256) and
        _unique_min(t[1]["medians"], c257) and t[1]["medians"][c256] > 50, ["upper_median", "tail_dropped", "index_one_low"] + list(LARGE))
    add("handover_257_256", [d257, d256], lambda a, t: a.tolist() == [c257, c256], ["upper_median", "tail_dropped", "index_one_low"] + list(LARGE))

    # ---- batch structure ------------------------------------------------------------------------------------------------------------------------------------
    def batch(name, counts, wrong):
        pts, want = [], []
        for n in counts:
            if n == 0:
                pts.append(np.zeros((0, 32), np.uint8)); want.append(-1)
            elif n < 6:
                pts.append(thermo([(40 + 3 * i * i, 9) for i in range(n)])); want.append(1 if n == 5 else 0)      # x = 40, 43, 52, 67, 88
            else:
                d, c = two_clusters(n)
                pts.append(d); want.append(c)
        add(name, pts, lambda a, t, want=want, counts=counts: a.tolist() == want and [x.get("N", 0) for x in t] == list(counts), wrong)

    EVEN_LARGE = ["upper_median"] + list(LARGE)
    batch("batch_interleaved", [0, 1, 5, 300, 0, 700, 2], EVEN_LARGE + ["last_minimum", "tail_dropped", "index_one_low"])
    batch("batch_1_large", [3, 301, 4], list(LARGE) + ["upper_median", "last_minimum", "tail_dropped"])
    batch("batch_4_large", [301, 2, 303, 305, 307], list(LARGE) + ["last_minimum", "tail_dropped"])
    batch("batch_5_large", [301, 303, 1, 305, 307, 309, 5], list(LARGE) + ["tail_dropped", "index_one_low"])
    for n_points in (3, 4, 5, 6):                                        # (n_points + 1) % 4 = 0, 1, 2, 3: the large list behind the rounded offsets
        counts = [1] * n_points
        counts[n_points // 2] = 257 + 2 * n_points
        counts[-1] = 291
        batch("batch_n%d" % n_points, counts, list(LARGE) + ["tail_dropped"])
    batch("batch_all_empty", [0, 0, 0, 0, 0], [])
    return out


def scenes():
    """Seeded batches of noisy-copy tracks (what the map holds): (name, off, desc).  Nothing is claimed about them but equality."""
    out = []
    for seed, counts in ((1, [2, 3, 4, 5, 8, 13, 21, 40, 64, 65, 100]), (2, [256, 0, 257, 1, 258, 12]), (3, [300, 127, 128, 129, 0, 0, 191, 192, 193, 450]),
                         (4, [int(c) for c in np.random.default_rng(40).integers(0, 30, 61)])):
        rng = np.random.default_rng(seed)
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        desc = np.zeros((int(off[-1]), 32), np.uint8)
        for p, n in enumerate(counts):
            base = rng.integers(0, 256, 32, dtype=np.uint8)
            desc[off[p]:off[p + 1]] = base ^ np.packbits(rng.random((n, 256)) < rng.choice([0.02, 0.1, 0.3]), axis=1)
        out.append(("scene_%d" % seed, off, desc))
    return out
