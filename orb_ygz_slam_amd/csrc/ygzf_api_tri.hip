// ygzf_api_tri.hip -- CreateNewMapPoints' per-pair triangulation, batched over neighbours (C ABI of libygzf, include/ygzf.h; product code: no
// CPU fallback, nothing from oracle/ is included or linked).  The problems of one call cross the link as one packed upload and one packed
// download (ProblemBlock, ygzf_ctx.h: [records | per distinct keyframe keys uRight depth cosStereo sigma2 scale | per problem idx1 idx2] up,
// [per problem x3d | status] down) around one launch of k_triangulate (tri_kernels.hip) and one synchronisation.
#include "ygzf_ctx.h"
#include "tri_math.h"

namespace {

struct TriKfSlots { ProblemBlock::Slot keys, right, depth, cosStereo, sigma2, scale; };

// the arrays of one keyframe as the caller names them: two records with the same arrays are one keyframe of the call
struct TriKfArrays {
    const void *keys, *right, *depth, *cosStereo, *scale, *sigma2;
    int n, nlevels;
    bool operator==(const TriKfArrays &o) const {
        return keys == o.keys && right == o.right && depth == o.depth && cosStereo == o.cosStereo && scale == o.scale && sigma2 == o.sigma2 && n == o.n &&
               nlevels == o.nlevels;
    }
};
TriKfArrays arrays_of(const ygzf_tri_kf &k) {
    return {k.view.keys, k.view.u_right, k.depth, k.cos_stereo, k.view.scale_factors, k.level_sigma2, k.view.n, k.view.nlevels};
}

int tri_levels(const ygzf_ctx *c, const ygzf_tri_kf &k) { return k.view.scale_factors ? k.view.nlevels : c->tab.cfg.nlevels; }

// null: the record is fine; else what is wrong with it
const char *check_kf(const ygzf_ctx *c, const ygzf_tri_kf &k) {
    if (k.view.n < 0) return "negative feature count";
    if (k.view.n > 0 && !k.view.keys) return "null keys";
    if (k.view.u_right && (!k.depth || !k.cos_stereo)) return "u_right without depth or cos_stereo";
    const int L = tri_levels(c, k);
    if (L <= 0) return "no scale levels";
    for (int i = 0; i < k.view.n; i++)
        if (k.view.keys[i].octave < 0 || k.view.keys[i].octave >= L) return "keypoint octave outside the scale tables";
    return nullptr;
}

void fill_kf(const ygzf_tri_kf &k, const ProblemBlock &B, const TriKfSlots &S, ygzf::TriKfDev &d) {
    d.k.fx = k.cam.fx; d.k.fy = k.cam.fy; d.k.cx = k.cam.cx; d.k.cy = k.cam.cy;
    d.k.invfx = k.invfx; d.k.invfy = k.invfy; d.k.mbf = k.cam.mbf;
    memcpy(d.k.Rcw, k.Rcw, sizeof d.k.Rcw);
    memcpy(d.k.tcw, k.tcw, sizeof d.k.tcw);
    memcpy(d.k.Ow, k.Ow, sizeof d.k.Ow);
    memcpy(d.k.q, k.Twc_q, sizeof d.k.q);
    memcpy(d.k.t, k.Twc_t, sizeof d.k.t);
    d.keys = B.dev<const ygzf_kp>(S.keys);
    d.uRight = k.view.u_right ? B.dev<const float>(S.right) : nullptr;
    d.depth = k.view.u_right ? B.dev<const float>(S.depth) : nullptr;
    d.cosStereo = k.view.u_right ? B.dev<const float>(S.cosStereo) : nullptr;
    d.sigma2 = B.dev<const float>(S.sigma2);
    d.scale = B.dev<const float>(S.scale);
}

}  // namespace

extern "C" {

int ygzf_triangulate_pairs(ygzf_ctx *c, const ygzf_tri_kf *kf1, float ratio_factor, int n_problems, const ygzf_tri_problem *p, float *const *x3d,
                           uint8_t *const *status) {
    using namespace ygzf;
    if (!c) return YGZF_ERR_INVALID;
    if (!kf1 || !p || !x3d || !status) return fail(c, YGZF_ERR_INVALID, "null argument");
    if (n_problems <= 0) return fail(c, YGZF_ERR_INVALID, "n_problems = %d: at least one problem is needed", n_problems);
    std::vector<int> live;   // the problems with pairs to triangulate
    long long totalPairs = 0;
    for (int k = 0; k < n_problems; k++) {
        if (p[k].n_pairs < 0) return fail(c, YGZF_ERR_INVALID, "problem %d: negative pair count", k);
        if (p[k].n_pairs == 0) continue;
        live.push_back(k);
        totalPairs += p[k].n_pairs;
    }
    if (live.empty()) return YGZF_OK;
    if (totalPairs > (1ll << 30)) return fail(c, YGZF_ERR_INVALID, "%lld pairs in one call", totalPairs);
    // the distinct keyframes of the call: kf1 first, then the live problems' kf2 in order of appearance
    std::vector<const ygzf_tri_kf *> kfs = {kf1};
    std::vector<int> kfOf(live.size());
    for (size_t j = 0; j < live.size(); j++) {
        const ygzf_tri_kf &k2 = p[live[j]].kf2;
        size_t u = 0;
        while (u < kfs.size() && !(arrays_of(*kfs[u]) == arrays_of(k2))) u++;
        if (u == kfs.size()) kfs.push_back(&k2);
        kfOf[j] = (int) u;
    }
    for (size_t u = 0; u < kfs.size(); u++)
        if (const char *what = check_kf(c, *kfs[u])) return u == 0 ? fail(c, YGZF_ERR_INVALID, "kf1: %s", what) : fail(c, YGZF_ERR_INVALID, "kf2: %s", what);
    for (size_t j = 0; j < live.size(); j++) {
        const int k = live[j];
        const ygzf_tri_problem &q = p[k];
        if (!q.idx1 || !q.idx2 || !x3d[k] || !status[k]) return fail(c, YGZF_ERR_INVALID, "problem %d: null array", k);
        for (int i = 0; i < q.n_pairs; i++) {
            if (q.idx1[i] < 0 || q.idx1[i] >= kf1->view.n) return fail(c, YGZF_ERR_INVALID, "problem %d: pair %d names feature %d of kf1 outside [0, %d)", k, i, q.idx1[i], kf1->view.n);
            if (q.idx2[i] < 0 || q.idx2[i] >= q.kf2.view.n) return fail(c, YGZF_ERR_INVALID, "problem %d: pair %d names feature %d of kf2 outside [0, %d)", k, i, q.idx2[i], q.kf2.view.n);
        }
    }
    HIPCHECK(c, hipSetDevice(c->device));
    const size_t L = live.size();
    struct Slots { ProblemBlock::Slot idx1, idx2, x3d, status; };
    std::vector<Slots> S(L);
    std::vector<TriKfSlots> KS(kfs.size());
    std::vector<std::vector<float>> tabs(2 * kfs.size());   // sigma2, scale per keyframe: alive until commit() has copied them
    ProblemBlock B(c, L * sizeof(TriProblemDev));
    for (size_t u = 0; u < kfs.size(); u++) {
        const ygzf_tri_kf &k = *kfs[u];
        const size_t n = (size_t) k.view.n;
        const int nl = tri_levels(c, k);
        std::vector<float> &sg = tabs[2 * u], &sf = tabs[2 * u + 1];
        sg.resize(nl);
        sf.resize(nl);
        for (int l = 0; l < nl; l++) {
            sf[l] = k.view.scale_factors ? k.view.scale_factors[l] : c->tab.scale[l];
            sg[l] = k.level_sigma2 ? k.level_sigma2[l] : sf[l] * sf[l];   // mvLevelSigma2[i] = mvScaleFactor[i] * mvScaleFactor[i]  (src/ORBextractor.cc:422)
        }
        KS[u].keys = B.in(k.view.keys, n * sizeof(ygzf_kp));
        KS[u].right = B.in(k.view.u_right, n * sizeof(float));
        KS[u].depth = B.in(k.view.u_right ? k.depth : nullptr, n * sizeof(float));
        KS[u].cosStereo = B.in(k.view.u_right ? k.cos_stereo : nullptr, n * sizeof(float));
        KS[u].sigma2 = B.in(sg.data(), (size_t) nl * sizeof(float));
        KS[u].scale = B.in(sf.data(), (size_t) nl * sizeof(float));
    }
    for (size_t j = 0; j < L; j++) {
        const int k = live[j];
        const size_t n = (size_t) p[k].n_pairs;
        S[j].idx1 = B.in(p[k].idx1, n * sizeof(int));
        S[j].idx2 = B.in(p[k].idx2, n * sizeof(int));
        S[j].x3d = B.out(x3d[k], 3 * n * sizeof(float));
        S[j].status = B.out(status[k], n);
    }
    int rc;
    if ((rc = B.commit())) return rc;
    TriProblemDev *probs = B.records<TriProblemDev>();
    int first = 0;
    for (size_t j = 0; j < L; j++) {
        const ygzf_tri_problem &q = p[live[j]];
        TriProblemDev &d = probs[j];
        fill_kf(q.kf2, B, KS[kfOf[j]], d.kf2);   // the pose and the camera are the problem's own; the arrays are its keyframe's
        d.idx1 = B.dev<const int>(S[j].idx1);
        d.idx2 = B.dev<const int>(S[j].idx2);
        d.x3d = B.dev<float>(S[j].x3d);
        d.status = B.dev<uint8_t>(S[j].status);
        d.nPairs = q.n_pairs;
        d.firstHyp = first;
        first += q.n_pairs;
    }
    if ((rc = B.upload())) return rc;
    TriPairArgs A;
    fill_kf(*kf1, B, KS[0], A.kf1);
    A.probs = B.dev_records<TriProblemDev>();
    A.nProblems = (int) L;
    A.totalPairs = (int) totalPairs;
    A.ratioFactor = ratio_factor;
    launch_triangulate(c->stream, A);
    HIPCHECK(c, hipGetLastError());
    return B.download();
}

}  // extern "C"
