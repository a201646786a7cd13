"""Constructed inputs for the vocabulary descent of Frame::ComputeBoW (ygzf_vocabulary_set / ygzf_bow_transform, k_bow_descend), numpy only.

restate() follows DBoW2's TemplatedVocabulary::transform(feature, word_id, weight, nid, levelsup) (TemplatedVocabulary.h:1240-1283): the
children of a node are visited in ascending node id (the loader's push_back order), the first nearest child wins (`d < best_d`), the key node is
the one reached at level L - levelsup, the key is root 0 where L - levelsup <= 0, and -- the project's definition, the reference leaves *nid
unassigned there -- where a leaf lies above that level the key is that leaf.  `form` swaps in ONE mistake a kernel or its table builder could
make (FORMS); every case lists in `wrong` the forms that must change its answer.

A vocabulary is the dict oracle.make_vocabulary returns (k, L, parent, is_leaf, desc, weight).  Centroids are built to exact distances: the
256 bits are groups of `width` bits, group g holds a thermometer code (its first v bits set), and the children of a level-(g + 1) node are their
parent's centroid plus a value in group g.  A query with values (v_0, v_1, ...) is |v_g - value(child)| plus the same constant from every child of
a level-(g + 1) node, so its path is chosen level by level.  Copies of one centroid give exact ties at zero and at non-zero distance.
"""
import numpy as np

FORMS = ("last_nearest",              # <= in place of <
         "later_chunk_wins",          # on a tie, a child at position >= 64 beats one of an earlier 64-chunk
         "chunk_local_position",      # the winner's position is taken modulo 64
         "consecutive_children",      # child p of a node is taken to be first_child_id + p
         "root_key_missing",          # for levelsup >= L the key is the level-1 node instead of 0
         "ragged_key_zero",           # a leaf above the key level gives key 0
         "last_word_ignored",         # bits 192..255 are not counted (a distance over three of the four 64-bit words)
         "distance_8_bits")           # the distance is kept in 8 bits: 256 becomes 0

_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int64)


def code(values, width):
    """thermometer groups: values[g] of the bits [g * width, (g + 1) * width) set from the group's start -> 32 bytes"""
    bits = np.zeros(256, np.uint8)
    for g, v in enumerate(values):
        assert 0 <= v <= width and (g + 1) * width <= 256
        bits[g * width:g * width + v] = 1
    return np.packbits(bits)


def children_lists(parent):
    """-> (order, off): the children of node i are order[off[i]:off[i + 1]], ascending node id"""
    parent = np.asarray(parent)
    order = np.argsort(parent[1:], kind="stable") + 1
    off = np.concatenate([[0], np.cumsum(np.bincount(parent[1:], minlength=len(parent)))]) if len(parent) > 1 else np.zeros(len(parent) + 1, np.int64)
    return order, off


def restate(voc, desc, levelsup, form=None, trace=None):
    """-> (leaf node id, key node id) per descriptor, int32.  trace receives one list per descriptor: a dict per level (ids, dist, pos)."""
    assert form is None or form in FORMS, form
    parent, vdesc = np.asarray(voc["parent"]), voc["desc"]
    n_nodes = len(parent)
    order, off = children_lists(parent)
    d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    nid_level = voc["L"] - levelsup
    leaf, key = np.zeros(len(d), np.int32), np.zeros(len(d), np.int32)
    nbytes = 24 if form == "last_word_ignored" else 32
    for i in range(len(d)):
        node, level, nid, steps = 0, 0, 0, []                            # if (nid_level <= 0) *nid = 0
        while off[node + 1] > off[node]:
            ids = order[off[node]:off[node + 1]]                         # m_nodes[final_id].children
            if form == "consecutive_children":
                ids = np.minimum(ids[0] + np.arange(len(ids)), n_nodes - 1)
            level += 1
            dist = _POP8[vdesc[ids, :nbytes] ^ d[i, :nbytes]].sum(1)
            if form == "distance_8_bits":
                dist = dist & 0xFF
            pos = int(np.argmin(dist))                                   # d < best_d: the first nearest child
            if form == "last_nearest":
                pos = len(dist) - 1 - int(np.argmin(dist[::-1]))
            if form == "later_chunk_wins":
                for base in range(64, len(dist), 64):
                    p = base + int(np.argmin(dist[base:base + 64]))
                    if dist[p] <= dist[pos]:
                        pos = p
            if form == "chunk_local_position":
                pos %= 64
            steps.append(dict(node=node, ids=ids, dist=dist, pos=pos))
            node = int(ids[pos])
            if level == nid_level or (form == "root_key_missing" and nid_level <= 0 and level == 1):
                nid = node
        if nid_level > 0 and level < nid_level:                          # a leaf above the key level: the key is that leaf
            nid = 0 if form == "ragged_key_zero" else node
        leaf[i], key[i] = node, nid
        if trace is not None:
            trace.append(steps)
    return leaf, key


# ---- trees ----------------------------------------------------------------------------------------------------------------------------------------------
def make_voc(parent, k, L, desc):
    parent = np.asarray(parent, np.int32)
    n = len(parent)
    is_leaf = (np.bincount(parent[1:], minlength=n) == 0).astype(np.uint8) if n > 1 else np.ones(1, np.uint8)
    ids = np.arange(n)
    weight = np.where((is_leaf > 0) & (ids % 19 != 18), 1.0 + (ids % 7) * 0.25, 0.0)       # a few stopped words, as the loaders produce
    return dict(k=k, L=L, parent=parent, is_leaf=is_leaf, desc=np.ascontiguousarray(desc, np.uint8), weight=weight)


def full_tree(k, L):
    """-> (parent, level, pos): the loaders' layout, the children of a node are consecutive ids"""
    parent, level, pos, frontier = [-1], [0], [0], [0]
    for lv in range(1, L + 1):
        nxt = []
        for p in frontier:
            for c in range(k):
                parent.append(p); level.append(lv); pos.append(c); nxt.append(len(parent) - 1)
        frontier = nxt
    return np.array(parent, np.int32), np.array(level), np.array(pos)


def value_voc(parent, level, pos, k, L, value, width):
    """the centroid of a node at level l, position p among its siblings: its parent's centroid with value(p) in group l - 1 (empty until then)"""
    table = {}
    desc = np.zeros((len(parent), 32), np.uint8)
    for i in range(1, len(parent)):
        key = (int(level[i]), int(pos[i]))
        if key not in table:
            vals = [0] * level[i]
            vals[level[i] - 1] = value(int(pos[i]))
            table[key] = code(vals, width)
        assert parent[i] < i
        desc[i] = desc[parent[i]] | table[key]
    return make_voc(parent, k, L, desc)


def positions(parent):
    """position of every node among its siblings, and its level"""
    order, off = children_lists(parent)
    pos, level = np.zeros(len(parent), np.int64), np.zeros(len(parent), np.int64)
    for node in range(len(parent)):
        pos[order[off[node]:off[node + 1]]] = np.arange(off[node + 1] - off[node])
    for i in range(1, len(parent)):                                      # (a parent's id may be larger than its child's in no tree here)
        assert parent[i] < i
        level[i] = level[parent[i]] + 1
    return pos, level


def tie_voc(k, L, tied):
    """k-ary, depth L: at every node the children at the positions `tied` carry the SAME centroid (value 10), the others sit far away (100 + p % 20)"""
    parent, level, pos = full_tree(k, L)
    return value_voc(parent, level, pos, k, L, lambda p: 10 if p in tied else 100 + p % 20, 128)


def ragged_tree():
    """k = 3, L = 3: node 1 is a leaf at level 1, node 2's children 4, 5, 6 are leaves at level 2, node 3's children 7, 8, 9 have the level-3 leaves 10..18"""
    parent = [-1, 0, 0, 0, 2, 2, 2, 3, 3, 3] + [7] * 3 + [8] * 3 + [9] * 3
    pos, level = positions(np.array(parent))
    return value_voc(np.array(parent, np.int32), level, pos, 3, 3, lambda p: 20 * p, 64)


def interleaved_31():
    """k = 5, L = 2: the level-2 nodes 6..30 are dealt to the level-1 nodes 1..5 in turn, so the children of node j are 5 + j, 10 + j, ..."""
    parent = np.array([-1] + [0] * 5 + [1 + i % 5 for i in range(25)], np.int32)
    pos, level = positions(parent)
    return value_voc(parent, level, pos, 5, 2, lambda p: 20 * p, 128)


def interleaved_7():
    parent = np.array([-1, 0, 0, 1, 2, 1, 2], np.int32)
    pos, level = positions(parent)
    return value_voc(parent, level, pos, 2, 2, lambda p: 40 * p, 128)


def root_alone():
    return make_voc([-1], 10, 0, np.zeros((1, 32), np.uint8))


class Case:
    def __init__(self, name, voc, desc, levelsup, reach, wrong, tree=None):
        self.name, self.voc, self.levelsup, self.reach, self.wrong = name, voc, levelsup, reach, tuple(wrong)
        self.desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        self.tree = tree or name                                         # cases of one `tree` share one vocabulary
        assert set(self.wrong) <= set(FORMS)

    def __repr__(self):
        return self.name


def _picked(trace):
    return [[s["pos"] for s in steps] for steps in trace]


def cases():
    out = []
    add = lambda *a, **k: out.append(Case(*a, **k))

    # ---- sibling ties: copies of one centroid, the query at distance 0 and at 3 -----------------------------------------------------------------
    def tie(name, k, tied, wrong):
        voc = tie_voc(k, 2, tied)
        q = np.stack([code([10, 0], 128), code([10, 10], 128), code([13, 13], 128)])
        def reach(leaf, nid, t):                                         # the tied children, and only they, are nearest: at distance 0 and above it
            return (_picked(t) == [[tied[0]] * 2] * 3 and [[int(s["dist"].min()) for s in steps] for steps in t] == [[0, 10], [10, 0], [16, 6]] and
                    all(np.nonzero(s["dist"] == s["dist"].min())[0].tolist() == list(tied) for steps in t for s in steps))
        add(name, voc, q, 1, reach, wrong)
    tie("tie_0_9_k10", 10, (0, 9), ["last_nearest"])
    tie("tie_3_4_k10", 10, (3, 4), ["last_nearest"])
    tie("tie_5_69_k70", 70, (5, 69), ["last_nearest", "later_chunk_wins"])
    tie("tie_63_64_k65", 65, (63, 64), ["last_nearest", "later_chunk_wins"])
    tie("tie_63_64_128_k129", 129, (63, 64, 128), ["last_nearest", "later_chunk_wins"])
    tie("twin_5_19_k20", 20, (5, 19), ["last_nearest"])                  # the ties of the k > 20 trees inside trees the reference's loader takes
    tie("twin_9_10_k20", 20, (9, 10), ["last_nearest"])
    tie("twin_3_4_19_k20", 20, (3, 4, 19), ["last_nearest"])

    # ---- branching: child p holds the value p; queries pick the first, the last and the children around the 64-chunk edges --------------------
    for k in (1, 2, 63, 64, 65, 128, 129):
        parent, level, pos = full_tree(k, 2)
        voc = value_voc(parent, level, pos, k, 2, lambda p: p, 128)
        want = sorted({p for p in (0, 1, 62, 63, 64, 65, 127, 128, k // 2, k - 2, k - 1) if 0 <= p < k})
        q = np.stack([code([a, want[-1 - i]], 128) for i, a in enumerate(want)])
        add("branch_%d" % k, voc, q, 1, lambda leaf, nid, t, want=want, k=k: _picked(t) == [[a, want[-1 - i]] for i, a in enumerate(want)] and
            (nid == 1 + np.array(want)).all() and (leaf == 1 + k + k * np.array(want) + np.array(want[::-1])).all() and
            all(len(s["ids"]) == k and int((s["dist"] == s["dist"].min()).sum()) == 1 for steps in t for s in steps),
            # (values above 64 in the second group reach bits 192..255; the 129-ary tree's query (0, 128) is 256 from the child holding 128)
            (["chunk_local_position"] if k > 64 else []) + (["last_word_ignored"] if k >= 128 else []) + (["distance_8_bits"] if k == 129 else []))
    assert len(full_tree(129, 2)[0]) == 16771

    # ---- distance 256: the query is the bitwise complement of a centroid ----------------------------------------------------------------------------
    parent, level, pos = full_tree(3, 1)
    voc = make_voc(parent, 3, 1, np.stack([np.zeros(32, np.uint8), code([40, 0], 128), code([64, 0], 128), code([128, 0], 128)]))
    add("complement_query", voc, ~voc["desc"][1:2], 0, lambda leaf, nid, t: t[0][0]["dist"].tolist() == [256, 232, 168] and leaf[0] == 3 == nid[0],
        ["distance_8_bits"])
    voc = make_voc(parent, 3, 1, np.stack([np.zeros(32, np.uint8), code([50, 64], 128), code([50, 100], 128), code([50, 128], 128)]))
    add("last_word_decides", voc, code([50, 128], 128)[None], 0, lambda leaf, nid, t: t[0][0]["dist"].tolist() == [64, 28, 0] and leaf[0] == 3,
        ["last_word_ignored"])

    # ---- sibling ids that interleave ------------------------------------------------------------------------------------------------------------------------
    voc = interleaved_7()
    q = np.stack([code([0, 40], 128), code([40, 40], 128), code([0, 0], 128), code([40, 0], 128)])
    add("interleaved_7", voc, q, 1, lambda leaf, nid, t: leaf.tolist() == [5, 6, 3, 4] and nid.tolist() == [1, 2, 1, 2] and
        t[0][1]["ids"].tolist() == [3, 5] and t[1][1]["ids"].tolist() == [4, 6], ["consecutive_children"], tree="interleaved_7")
    voc = interleaved_31()
    q = np.stack([code([20 * a, 20 * b], 128) for a in range(5) for b in range(5)])
    add("interleaved_31", voc, q, 1, lambda leaf, nid, t: leaf.tolist() == [6 + a + 5 * b for a in range(5) for b in range(5)] and
        t[7][1]["ids"].tolist() == [7, 12, 17, 22, 27], ["consecutive_children"])

    # ---- the key level: levelsup 0, 1, L - 1, L, L + 1 on a full and on a ragged tree ---------------------------------------------------------------------
    parent, level, pos = full_tree(4, 3)
    voc = value_voc(parent, level, pos, 4, 3, lambda p: 20 * p, 64)
    q = np.stack([code([20 * a, 20 * b, 20 * c], 64) for a, b, c in ((0, 0, 0), (3, 3, 3), (1, 2, 3), (2, 0, 1), (3, 1, 0))])
    lv = level
    for levelsup in (0, 1, 2, 3, 4):
        def reach(leaf, nid, t, levelsup=levelsup):
            want = 3 - levelsup
            path = [[int(s["ids"][s["pos"]]) for s in steps] for steps in t]
            return all(len(p) == 3 for p in path) and nid.tolist() == [p[want - 1] if want > 0 else 0 for p in path] and (lv[leaf] == 3).all()
        add("full_levelsup_%d" % levelsup, voc, q, levelsup, reach, ["root_key_missing"] if levelsup >= 3 else [], tree="full_4_3")
    voc = ragged_tree()
    q = np.stack([code([0, 0, 0], 64), code([20, 40, 0], 64), code([40, 20, 40], 64), code([40, 0, 0], 64), code([20, 0, 20], 64)])
    for levelsup in (0, 1, 2, 3, 4):
        def reach(leaf, nid, t, levelsup=levelsup):
            want = 3 - levelsup
            key = {3: [1, 6, 15, 10, 4], 2: [1, 6, 8, 7, 4], 1: [1, 2, 3, 3, 2]}.get(want, [0] * 5)
            return leaf.tolist() == [1, 6, 15, 10, 4] and [len(s) for s in t] == [1, 2, 3, 3, 2] and nid.tolist() == key
        add("ragged_levelsup_%d" % levelsup, voc, q, levelsup, reach,
            ["root_key_missing"] if levelsup >= 3 else ["ragged_key_zero"] if levelsup <= 1 else [], tree="ragged")

    # ---- the root alone --------------------------------------------------------------------------------------------------------------------------------
    rng = np.random.default_rng(5)
    for levelsup in (0, 4):
        add("root_alone_levelsup_%d" % levelsup, root_alone(), rng.integers(0, 256, (6, 32), dtype=np.uint8), levelsup,
            lambda leaf, nid, t: not leaf.any() and not nid.any() and all(s == [] for s in t), [], tree="root_alone")

    # ---- batch sizes: four descriptors per workgroup ----------------------------------------------------------------------------------------------------
    parent, level, pos = full_tree(10, 2)
    voc = value_voc(parent, level, pos, 10, 2, lambda p: 6 * p, 128)
    for n in (1, 3, 4, 5, 257):
        ab = [((7 * i + 3) % 10, (3 * i + 1) % 10) for i in range(n)]
        q = np.stack([code([6 * a + (i % 3), 6 * b + 2 - (i % 3)], 128) for i, (a, b) in enumerate(ab)])      # up to 2 off the centroid: still nearest
        add("batch_%d" % n, voc, q, 1, lambda leaf, nid, t, ab=ab: leaf.tolist() == [11 + 10 * a + b for a, b in ab] and nid.tolist() == [1 + a for a, _ in ab],
            [], tree="full_10_2")
    return out


def reference_loadable(voc):
    """what the reference's text loader takes (TemplatedVocabulary.h:1383) and what its descent can walk (a root with children)"""
    return voc["k"] <= 20 and 1 <= voc["L"] <= 10 and len(voc["parent"]) > 1


def key_defined(voc, leaf, levelsup):
    """False for the descriptors whose leaf lies above the key level: the reference leaves *nid unassigned there"""
    _, level = positions(np.asarray(voc["parent"]))
    want = voc["L"] - levelsup
    return (want <= 0) | (level[np.asarray(leaf)] >= want)
