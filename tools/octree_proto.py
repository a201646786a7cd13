#!/usr/bin/env python3
"""Array/range formulation of ORBextractor::DistributeOctTree (prototype of the HIP kernel k_octree).

Points get a 'path key' (root index, then 2 bits per subdivision: bit0 = x >= midX, bit1 = y >= midY, following
ExtractorNode::DivideNode's ceil-halving, reference src/ORBextractor.cc:479-531).  After sorting by key every octree
node is a contiguous range, so the breadth-first passes of :578-700 operate on (lo, cnt, depth) triples only.
Validated against the oracle's literal std::list restatement in tests/test_octree_proto.py.

The kernel's sort plan orders the keys on their top 14 bits first (distribute(prefix_bits=14), distribute_restarting) and sorts its keypoints for
k_describe by a compact tile key (tile_keys): tests/test_octree_prefix_sort_cpu.py.
    python tools/octree_proto.py --restart-share [frames]    how many (level, frame) pairs of bench.py's two 752x480 clips would start over
"""
import math
import os
import numpy as np


def path_keys(xs, ys, W, H, nIni, hX, D):
    keys = np.zeros(len(xs), np.int64)
    for i, (x, y) in enumerate(zip(xs.tolist(), ys.tolist())):
        root = int(np.float32(x) / np.float32(hX))
        root = min(root, nIni - 1)
        xl = int(np.float32(hX) * np.float32(root))
        xr = int(np.float32(hX) * np.float32(root + 1))
        yl, yr = 0, H
        k = root
        for _ in range(D):
            mx = xl + ((xr - xl + 1) >> 1)
            my = yl + ((yr - yl + 1) >> 1)
            bx = 1 if x >= mx else 0
            by = 1 if y >= my else 0
            if bx: xl = mx
            else: xr = mx
            if by: yl = my
            else: yr = my
            k = (k << 2) | (by << 1) | bx
        keys[i] = k
    return keys


PREFIX_BITS = 14   # k_octree's prefix sort: two radix digits of seven bits (csrc/extract_kernels.hip: 2 * kRadixBits)


def key_layout(minX, maxX, minY, maxY):
    """(nIni, hX, D, keyBits) of a level's path keys: root index on ceil(log2 nIni) bits, then two bits per subdivision"""
    W, H = maxX - minX, maxY - minY
    nIni = int(math.floor(np.float32(W) / np.float32(H) + 0.5))  # std::round of a positive float
    nIni = max(nIni, 1)
    hX = np.float32(W) / np.float32(nIni)
    rootW = max(int(np.float32(hX) * np.float32(i + 1)) - int(np.float32(hX) * np.float32(i)) for i in range(nIni))
    D = max(1, math.ceil(math.log2(max(rootW, H, 2)))) + 1
    rootBits = 0
    while (1 << rootBits) < nIni:
        rootBits += 1
    return nIni, hX, D, rootBits + 2 * D


def low_bit(keyBits, prefix_bits=PREFIX_BITS):
    """first key bit the prefix sort orders (0: the key is no longer than the prefix, the sort is the full one)"""
    return keyBits - prefix_bits if keyBits > prefix_bits else 0


def tile_keys(kx, ky, w):
    """processing-order keys of keypoints at (kx, ky) of a level image w px wide: (the 12-bit key, the compact row-major tile index) -- k_octree sorts
    on the second one; both order the 64x64-px tiles alike while kx < w"""
    kx = np.asarray(kx, np.int64); ky = np.asarray(ky, np.int64)
    tilesX = (w + 63) >> 6
    return ((ky >> 6) << 6) | (kx >> 6), (ky >> 6) * tilesX + (kx >> 6)


def tile_key_bits(w, h):
    """bits of the compact tile key of a w x h level: what tilesX * tilesY - 1 needs"""
    n, bits = ((w + 63) >> 6) * ((h + 63) >> 6), 0
    while (1 << bits) < n:
        bits += 1
    return bits


def distribute(xs, ys, resp, minX, maxX, minY, maxY, N, prefix_bits=None, info=None):
    """prefix_bits: order the keys (stably) on their top prefix_bits bits only, as k_octree's first attempt at a level does; a subdivision that
    would read a digit below them gets the kernel's dummy answer and sets info["overflow"] -- the result then means nothing and the level is
    distributed again on fully sorted keys (distribute_restarting).  info (a dict) receives D, keyBits, lowBit, overflow and `deepest`: the
    largest dep + 1 whose digit the kernel consults -- every node with more than one point in a full pass and EVERY expandable node at the
    start of an expand round (the kernel takes the child boundaries of all of them at once, before it knows where the round breaks off)."""
    xs = np.asarray(xs); ys = np.asarray(ys); resp = np.asarray(resp)
    M = len(xs)
    W, H = maxX - minX, maxY - minY
    nIni, hX, D, keyBits = key_layout(minX, maxX, minY, maxY)
    lowBit = low_bit(keyBits, prefix_bits) if prefix_bits else 0
    if info is None:
        info = {}
    info.update(D=D, keyBits=keyBits, lowBit=lowBit, overflow=False, deepest=0)
    keys = path_keys(xs, ys, W, H, nIni, hX, D)
    order = np.argsort(keys >> lowBit, kind="stable")
    skeys = keys[order]

    def consult(depth):
        info["deepest"] = max(info["deepest"], depth + 1)

    def children(lo, cnt, depth):
        shift = 2 * (D - (depth + 1))
        consult(depth)
        if shift < lowBit:                     # oct_bounds: a digit the prefix sort did not order
            info["overflow"] = True
            return [(lo, cnt, depth + 1), (lo + cnt, 0, depth + 1), (lo + cnt, 0, depth + 1), (lo + cnt, 0, depth + 1)]
        dig = (skeys[lo:lo + cnt] >> shift) & 3
        b = [lo + int(np.searchsorted(dig, c, side="left")) for c in (1, 2, 3)]
        bounds = [lo] + b + [lo + cnt]
        return [(bounds[c], bounds[c + 1] - bounds[c], depth + 1) for c in range(4)]

    # initial roots (list order = root order), empty ones dropped
    rootdig = skeys >> (2 * D)
    nodes = []
    for r in range(nIni):
        lo = int(np.searchsorted(rootdig, r, side="left"))
        hi = int(np.searchsorted(rootdig, r, side="right"))
        if hi > lo:
            nodes.append((lo, hi - lo, 0))
    finish = False
    while not finish:
        prev = len(nodes)
        kids_blocks, singles, E = [], [], []
        for (lo, cnt, d) in nodes:           # front to back
            if cnt == 1:
                singles.append((lo, cnt, d))
            else:
                ch = [c for c in children(lo, cnt, d) if c[1] > 0]
                kids_blocks.append(ch)
                E.extend(c for c in ch if c[1] > 1)   # creation order: n1..n4
        newnodes = []
        for ch in reversed(kids_blocks):
            newnodes.extend(reversed(ch))     # push_front order: n4 ... n1 at the front
        nodes = newnodes + singles
        nToExpand = len(E)
        if len(nodes) >= N or len(nodes) == prev:
            finish = True
        elif len(nodes) + 3 * nToExpand > N:
            while not finish:
                prev = len(nodes)
                for e in E:                  # the kernel takes every expandable node's boundaries before the round's break is known
                    consult(e[2])
                    if 2 * (D - (e[2] + 1)) < lowBit:
                        info["overflow"] = True
                # descending (size, creation seq)
                idx = sorted(range(len(E)), key=lambda j: (E[j][1], j))
                newE, front, processed = [], [], set()
                size = len(nodes)
                for j in reversed(idx):
                    ch = [c for c in children(*E[j]) if c[1] > 0]
                    front = list(reversed(ch)) + front
                    newE.extend(c for c in ch if c[1] > 1)
                    processed.add(E[j])
                    size += len(ch) - 1
                    if size >= N:
                        break
                nodes = front + [n for n in nodes if n not in processed]
                E = newE
                if len(nodes) >= N or len(nodes) == prev:
                    finish = True
    out = []
    for (lo, cnt, d) in nodes:
        ids = order[lo:lo + cnt]
        best = max(ids.tolist(), key=lambda i: (resp[i], -i))
        out.append(best)
    info["nodes"] = list(nodes)
    return np.array(out, np.int32)


def distribute_restarting(xs, ys, resp, minX, maxX, minY, maxY, N, info=None):
    """what k_octree's sort plan does: the prefix sort first; if that tree overflowed, the keys once more on every bit and the tree from its
    roots (the kernel sorts the prefix-sorted pairs again, which ends in the full sort's order: equal prefixes were in candidate order).
    info["restarted"] says which."""
    if info is None:
        info = {}
    out = distribute(xs, ys, resp, minX, maxX, minY, maxY, N, prefix_bits=PREFIX_BITS, info=info)
    info["restarted"] = info["overflow"]
    if info["overflow"]:
        out = distribute(xs, ys, resp, minX, maxX, minY, maxY, N, info={})
    return out


def restart_share(frames, nfeatures=1000, scale=1.2, nlevels=8, ini=20, mn=7):
    """(level, frame) pairs of a clip whose prefix-sorted attempt would start over, with the candidates of the oracle's FAST.
    -> (restarts per level, pairs per level, deepest dep + 1 consulted per level, D and lowBit per level)"""
    from oracle import oracle_py as O
    ex = O.Extractor(nfeatures, scale, nlevels, ini, mn)
    nfeat = ex.tables()["nfeat"]
    restarts, pairs, deepest, layout = [0] * nlevels, [0] * nlevels, [0] * nlevels, [None] * nlevels
    for img in frames:
        pyr = ex.pyramid(np.ascontiguousarray(img))
        for l in range(nlevels):
            xs, ys, sc = ex.cell_candidates(l)
            if len(xs) == 0:
                continue
            lw, lh = pyr[l].shape[1], pyr[l].shape[0]
            info = {}
            distribute(xs, ys, sc, 16, lw - 16, 16, lh - 16, int(nfeat[l]), info=info)
            lowBit = low_bit(info["keyBits"])
            pairs[l] += 1
            restarts[l] += 2 * (info["D"] - info["deepest"]) < lowBit
            deepest[l] = max(deepest[l], info["deepest"])
            layout[l] = (info["D"], info["keyBits"], lowBit)
    return restarts, pairs, deepest, layout


def report_restart_shares(nframes):
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    for name, frames in (("bench.py make_frames (synthetic)", bench.make_frames(nframes, 752, 480)),
                         ("bench.py make_frames_test1png (real image)", bench.make_frames_test1png(nframes, 752, 480))):
        r, p, d, lay = restart_share(frames)
        print("%s, %d frames of 752x480, 8 levels, 1000 features: %d of %d (level, frame) pairs would restart (%.2f %%)" % (
            name, nframes, sum(r), sum(p), 100.0 * sum(r) / max(1, sum(p))))
        for l in range(len(r)):
            if lay[l]:
                print("  level %d: D %2d keyBits %2d lowBit %d (digits down to dep + 1 = %d are sorted)  deepest dep + 1 consulted %2d  restarts %d / %d" % (
                    l, lay[l][0], lay[l][1], lay[l][2], lay[l][0] - (lay[l][2] + 1) // 2, d[l], r[l], p[l]))


if __name__ == "__main__":
    import os, sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if len(sys.argv) > 1 and sys.argv[1] == "--restart-share":   # [frames per clip, default 32]
        report_restart_shares(int(sys.argv[2]) if len(sys.argv) > 2 else 32)
        sys.exit(0)
    from oracle import oracle_py as O
    from orb_ygz_slam_amd.synth import synth_frame
    ex = O.Extractor(1000, 1.2, 8, 20, 7)
    tot = 0
    for seed in range(6):
        for (w, h) in ((640, 480), (752, 480), (333, 517)):
            img = synth_frame(seed, w, h)
            pyr = ex.pyramid(img)
            for l in range(8):
                xs, ys, sc = ex.cell_candidates(l)
                if len(xs) == 0: continue
                lw, lh = pyr[l].shape[1], pyr[l].shape[0]
                for N in (ex.tables()["nfeat"][l], 5, 1, 40, 3000):
                    a = ex.octree(xs, ys, sc, 16, lw - 16, 16, lh - 16, int(N))
                    b = distribute(xs, ys, sc, 16, lw - 16, 16, lh - 16, int(N))
                    assert len(a) == len(b) and (a == b).all(), (seed, w, h, l, N, len(a), len(b))
                    tot += 1
    print("octree prototype == oracle on", tot, "cases")
