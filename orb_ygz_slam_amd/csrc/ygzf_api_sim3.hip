// ygzf_api_sim3.hip -- Sim3Solver's RANSAC hypotheses, batched over solvers (C ABI of libygzf, include/ygzf.h; product code: no CPU fallback,
// nothing from oracle/ is included or linked).  The problems of one call cross the link as one packed upload and one packed download
// (ProblemBlock, ygzf_ctx.h: [records | per problem X1 X2 maxErr1 maxErr2 samples] up, [per problem hyp | counts | bits] down) around one
// launch of k_sim3_ransac (sim3_kernels.hip) and one synchronisation.
#include "ygzf_ctx.h"
#include "sim3_math.h"

extern "C" {

int ygzf_sim3_ransac(ygzf_ctx *c, int n_problems, const ygzf_sim3_problem *p, float *const *hyp, int *const *n_inliers, uint64_t *const *inlier_bits) {
    if (!c) return YGZF_ERR_INVALID;
    if (!p || !hyp || !n_inliers) return fail(c, YGZF_ERR_INVALID, "null argument");
    if (n_problems <= 0) return fail(c, YGZF_ERR_INVALID, "n_problems = %d: at least one problem is needed", n_problems);
    std::vector<int> live;   // the problems with hypotheses to evaluate
    long long totalHyp = 0;
    for (int k = 0; k < n_problems; k++) {
        const ygzf_sim3_problem &q = p[k];
        if (q.n_hyp < 0) return fail(c, YGZF_ERR_INVALID, "problem %d: negative hypothesis count", k);
        if (q.n_hyp == 0) continue;
        if (q.n < 3) return fail(c, YGZF_ERR_INVALID, "problem %d: %d correspondences, a hypothesis needs 3", k, q.n);
        if (!q.X3Dc1 || !q.X3Dc2 || !q.max_err1 || !q.max_err2 || !q.samples || !hyp[k] || !n_inliers[k]) return fail(c, YGZF_ERR_INVALID, "problem %d: null array", k);
        for (int h = 0; h < q.n_hyp; h++) {
            const int *s = q.samples + 3 * (size_t) h;
            for (int j = 0; j < 3; j++)
                if (s[j] < 0 || s[j] >= q.n) return fail(c, YGZF_ERR_INVALID, "problem %d: hypothesis %d samples index %d outside [0, %d)", k, h, s[j], q.n);
            if (s[0] == s[1] || s[0] == s[2] || s[1] == s[2]) return fail(c, YGZF_ERR_INVALID, "problem %d: hypothesis %d repeats an index", k, h);
        }
        live.push_back(k);
        totalHyp += q.n_hyp;
    }
    if (live.empty()) return YGZF_OK;
    if (totalHyp > (1ll << 30)) return fail(c, YGZF_ERR_INVALID, "%lld hypotheses in one call", totalHyp);
    HIPCHECK(c, hipSetDevice(c->device));
    const size_t L = live.size();
    struct Slots { ProblemBlock::Slot X1, X2, e1, e2, samples, hyp, counts, bits; };
    std::vector<Slots> S(L);
    ProblemBlock B(c, L * sizeof(Sim3ProblemDev));
    for (size_t j = 0; j < L; j++) {
        const int k = live[j];
        const ygzf_sim3_problem &q = p[k];
        const size_t n = (size_t) q.n, nh = (size_t) q.n_hyp, words = (n + 63) / 64;
        uint64_t *bits = inlier_bits ? inlier_bits[k] : nullptr;
        S[j].X1 = B.in(q.X3Dc1, 3 * n * sizeof(float));
        S[j].X2 = B.in(q.X3Dc2, 3 * n * sizeof(float));
        S[j].e1 = B.in(q.max_err1, n * sizeof(float));
        S[j].e2 = B.in(q.max_err2, n * sizeof(float));
        S[j].samples = B.in(q.samples, 3 * nh * sizeof(int));
        S[j].hyp = B.out(hyp[k], nh * sim3::kHypFloats * sizeof(float));
        S[j].counts = B.out(n_inliers[k], nh * sizeof(int));
        S[j].bits = B.out(bits, bits ? nh * words * sizeof(uint64_t) : 0);
    }
    int rc;
    if ((rc = B.commit())) return rc;
    Sim3ProblemDev *probs = B.records<Sim3ProblemDev>();
    int first = 0;
    for (size_t j = 0; j < L; j++) {
        const ygzf_sim3_problem &q = p[live[j]];
        Sim3ProblemDev &d = probs[j];
        d.X1 = B.dev<const float>(S[j].X1);
        d.X2 = B.dev<const float>(S[j].X2);
        d.maxErr1 = B.dev<const float>(S[j].e1);
        d.maxErr2 = B.dev<const float>(S[j].e2);
        d.samples = B.dev<const int>(S[j].samples);
        d.hyp = B.dev<float>(S[j].hyp);
        d.nInliers = B.dev<int>(S[j].counts);
        d.bits = S[j].bits.bytes ? B.dev<uint64_t>(S[j].bits) : nullptr;
        d.n = q.n; d.nHyp = q.n_hyp; d.fixScale = q.fix_scale ? 1 : 0;
        d.firstHyp = first;
        first += q.n_hyp;
        memcpy(d.K1, q.K1, sizeof d.K1);
        memcpy(d.K2, q.K2, sizeof d.K2);
    }
    if ((rc = B.upload())) return rc;
    Sim3Args A;
    A.probs = B.dev_records<Sim3ProblemDev>();
    A.nProblems = (int) L;
    A.totalHyp = (int) totalHyp;
    launch_sim3_ransac(c->stream, A);
    HIPCHECK(c, hipGetLastError());
    return B.download();
}

}  // extern "C"
