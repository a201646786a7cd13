// tri_apply_cpu.cc -- CPU test of host/TriangulateApply.h (tests/test_tri_host_progs.py): on two copies of one seeded mock map, (a) the
// neighbour loop of LocalMapping::CreateNewMapPoints as the reference runs it -- each neighbour searched against the slots as they are by then --
// and (b) triangulate_apply over one snapshot must create the same points in the same order and leave the same slots.  Also runs (c)
// triangulate_apply without the drop rule and reports whether it diverged.
//   tri_apply_cpu seed shared dup stop
//     shared   how many neighbours match one KF1 feature in the scenes' overlap block: 1 (no feature is shared), 2 or 3
//     dup      1: a neighbour matches one of its features to two KF1 features
//     stop     the neighbour before which CheckNewKeyFrames() turns true; -1: never
// The mock search keeps what the exactness argument of TriangulateApply.h rests on: a candidate (idx1, idx2) of neighbour j is matched iff
// neither slot holds a MapPoint, independently of every other candidate.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "TriangulateApply.h"

namespace {

struct MapPoint { int id; int kf2, idx1, idx2; float x[3]; };
struct KeyFrame {
    int id = 0, N = 0;
    bool gate = true;
    std::vector<MapPoint *> slots;
    MapPoint *GetMapPoint(size_t i) const { return slots[i]; }
    void AddMapPoint(MapPoint *p, size_t i) { slots[i] = p; }
};
struct Cand { size_t idx1, idx2; bool accepted; float x[3]; };
struct World {
    KeyFrame cur;
    std::vector<KeyFrame> neigh;
    std::vector<std::vector<Cand>> cands;   // per neighbour, ascending idx1, each idx1 once
    std::vector<MapPoint *> recent;         // mlpRecentAddedMapPoints
    std::vector<MapPoint> pre;              // the points the map held before (storage reserved up front: pointers stay valid)
    ~World() { for (MapPoint *p : recent) delete p; }
};

struct Lcg {
    unsigned s;
    unsigned next() { s = s * 1664525u + 1013904223u; return s >> 8; }
    bool chance(unsigned percent) { return next() % 100 < percent; }
};

const int kN = 80, kNeigh = 5;

void make_world(World &w, unsigned seed, int shared, bool dup) {
    Lcg g{seed * 2654435761u + 17u};
    w.cur.N = kN;
    w.cur.slots.assign(kN, nullptr);
    w.neigh.resize(kNeigh);
    w.cands.resize(kNeigh);
    w.pre.reserve((size_t) kN * (kNeigh + 1));
    auto fill = [&](KeyFrame &k) {
        for (int i = 0; i < k.N; i++)
            if (g.chance(20)) { w.pre.push_back({-1 - (int) w.pre.size(), -1, -1, -1, {0, 0, 0}}); k.slots[i] = &w.pre.back(); }
    };
    fill(w.cur);
    for (int j = 0; j < kNeigh; j++) {
        KeyFrame &k = w.neigh[j];
        k.id = j + 1; k.N = kN; k.slots.assign(kN, nullptr);
        k.gate = j != 2;   // one neighbour fails the baseline gate
        fill(k);
        for (int i = 0; i < kN; i++) {
            // KF1 features 0 .. 19 are the overlap block: matched by the first `shared` neighbours that pass the gate (0, 1, 3); the others are
            // matched by neighbour i % kNeigh only
            const int order[3] = {0, 1, 3};
            bool mine = false;
            if (i < 20) { for (int s = 0; s < shared; s++) mine = mine || order[s] == j; }
            else mine = i % kNeigh == j;
            if (!mine || g.chance(15)) continue;
            Cand c;
            c.idx1 = (size_t) i;
            c.idx2 = (size_t) (g.next() % kN);
            c.accepted = g.chance(70);
            for (int a = 0; a < 3; a++) c.x[a] = (float) (g.next() % 1000) * 0.01f + (float) j;
            w.cands[j].push_back(c);
        }
        if (dup && w.cands[j].size() >= 4) {   // two accepted pairs on one free slot of the neighbour
            size_t free2 = 0;
            while (free2 < (size_t) kN && k.slots[free2]) free2++;
            Cand &a = w.cands[j][1], &b = w.cands[j][3];
            a.idx2 = b.idx2 = free2;
            a.accepted = b.accepted = true;
        }
    }
}

// SearchForTriangulation as the mock has it
void search(const std::vector<Cand> &cands, const std::vector<uint8_t> &has1, const std::vector<uint8_t> &has2,
            std::vector<std::pair<size_t, size_t>> &pairs, std::vector<const Cand *> *which = nullptr) {
    for (const Cand &c : cands)
        if (!has1[c.idx1] && !has2[c.idx2]) {
            pairs.push_back({c.idx1, c.idx2});
            if (which) which->push_back(&c);
        }
}
std::vector<uint8_t> slots_of(const KeyFrame &k) {
    std::vector<uint8_t> h(k.N);
    for (int i = 0; i < k.N; i++) h[i] = k.slots[i] ? 1 : 0;
    return h;
}
void create(World &w, KeyFrame *kf2, size_t idx1, size_t idx2, const float *x) {   // :1197-1214
    MapPoint *p = new MapPoint{(int) w.recent.size(), kf2->id, (int) idx1, (int) idx2, {x[0], x[1], x[2]}};
    w.cur.AddMapPoint(p, idx1);
    kf2->AddMapPoint(p, idx2);
    w.recent.push_back(p);
}

struct Poll {
    int stop, calls = 0;
    bool operator()() { calls++; return stop >= 0 && calls >= stop; }   // the call before neighbour j is call number j
};

// the loop as the reference runs it
int sequential(World &w, int stop) {
    Poll poll{stop};
    int nnew = 0;
    for (size_t j = 0; j < w.neigh.size(); j++) {
        if (j > 0 && poll()) return nnew;
        KeyFrame &k2 = w.neigh[j];
        if (!k2.gate) continue;
        std::vector<std::pair<size_t, size_t>> pairs;
        std::vector<const Cand *> which;
        search(w.cands[j], slots_of(w.cur), slots_of(k2), pairs, &which);
        for (const Cand *c : which) {
            if (!c->accepted) continue;
            create(w, &k2, c->idx1, c->idx2, c->x);
            nnew++;
        }
    }
    return nnew;
}

ygzf_host::TriangulateApplyResult batched(World &w, int stop, bool drop) {
    std::vector<KeyFrame *> neigh;
    for (KeyFrame &k : w.neigh) neigh.push_back(&k);
    Poll poll{stop};
    auto gate = [](KeyFrame *k) { return k->gate; };
    auto srch = [&](KeyFrame *k, const std::vector<uint8_t> &h1, const std::vector<uint8_t> &h2, std::vector<std::pair<size_t, size_t>> &pairs) {
        search(w.cands[k->id - 1], h1, h2, pairs);
        return true;
    };
    auto query = [&](const std::vector<KeyFrame *> &kfs, const std::vector<std::vector<std::pair<size_t, size_t>>> &pairs,
                     std::vector<std::vector<uint8_t>> &accepted, std::vector<std::vector<float>> &x3d) {
        for (size_t r = 0; r < kfs.size(); r++)
            for (size_t i = 0; i < pairs[r].size(); i++)
                for (const Cand &c : w.cands[kfs[r]->id - 1])
                    if (c.idx1 == pairs[r][i].first) {
                        accepted[r][i] = c.accepted;
                        for (int a = 0; a < 3; a++) x3d[r][3 * i + a] = c.x[a];
                    }
        return true;
    };
    auto mk = [&](KeyFrame *k, size_t i1, size_t i2, const float *x) { create(w, k, i1, i2, x); };
    return ygzf_host::triangulate_apply<KeyFrame, MapPoint>(&w.cur, neigh, gate, srch, query, mk, poll, drop);
}

int slot_id(const MapPoint *p) { return p ? p->id : -1000000; }

// -> the number of differences
int compare(const World &a, const World &b) {
    int bad = 0;
    if (a.recent.size() != b.recent.size()) bad++;
    for (size_t i = 0; i < a.recent.size() && i < b.recent.size(); i++) {
        const MapPoint &p = *a.recent[i], &q = *b.recent[i];
        if (p.kf2 != q.kf2 || p.idx1 != q.idx1 || p.idx2 != q.idx2 || p.x[0] != q.x[0] || p.x[1] != q.x[1] || p.x[2] != q.x[2]) bad++;
    }
    for (int i = 0; i < kN; i++) bad += slot_id(a.cur.slots[i]) != slot_id(b.cur.slots[i]);
    for (size_t j = 0; j < a.neigh.size(); j++)
        for (int i = 0; i < kN; i++) bad += slot_id(a.neigh[j].slots[i]) != slot_id(b.neigh[j].slots[i]);
    return bad;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 5) { std::fprintf(stderr, "usage: tri_apply_cpu seed shared dup stop\n"); return 2; }
    const unsigned seed = (unsigned) std::atoi(argv[1]);
    const int shared = std::atoi(argv[2]), dup = std::atoi(argv[3]), stop = std::atoi(argv[4]);
    World a, b, c;
    make_world(a, seed, shared, dup != 0);
    make_world(b, seed, shared, dup != 0);
    make_world(c, seed, shared, dup != 0);
    const int nA = sequential(a, stop);
    const ygzf_host::TriangulateApplyResult rb = batched(b, stop, true), rc = batched(c, stop, false);
    int overwritten = 0;   // points whose slot in their neighbour a later point of the same neighbour took
    for (const MapPoint *p : a.recent) overwritten += a.neigh[p->kf2 - 1].slots[p->idx2] != p;
    const int bad = compare(a, b) + (nA != rb.nnew ? 1 : 0);
    const int diverged = compare(a, c) + (nA != rc.nnew ? 1 : 0);
    std::printf("seed %u created %d searched %lld dropped %lld overwritten %d stopped_at %d diverged %d\n", seed, nA, rb.searchedPairs, rb.dropped,
                overwritten, rb.stoppedAt, diverged);
    if (!rb.ok || bad) { std::printf("%d differences\n", bad); return 1; }
    std::printf("triangulate apply ok\n");
    return 0;
}
