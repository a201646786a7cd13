// ygzf_api_sim3.hip -- Sim3Solver's RANSAC hypotheses, batched over solvers (C ABI of libygzf, include/ygzf.h; product code: no CPU fallback,
// nothing from oracle/ is included or linked).  The problems of one call cross the link as one packed upload and one packed download around one
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
    // one host block each way, as ygzf_pose_optimization lays its problems out: [records | per problem X1 X2 maxErr1 maxErr2 samples] up,
    // [per problem hyp | counts | bits] down
    const size_t L = live.size();
    auto al = [](size_t b) { return (b + 63) & ~(size_t) 63; };
    std::vector<size_t> oX1(L), oX2(L), oE1(L), oE2(L), oS(L), rHyp(L), rCnt(L), rBits(L);
    size_t inBytes = al(L * sizeof(Sim3ProblemDev)), outBytes = 0;
    for (size_t j = 0; j < L; j++) {
        const ygzf_sim3_problem &q = p[live[j]];
        const size_t n = (size_t) q.n, nh = (size_t) q.n_hyp, words = (n + 63) / 64;
        oX1[j] = inBytes; inBytes += al(3 * n * sizeof(float));
        oX2[j] = inBytes; inBytes += al(3 * n * sizeof(float));
        oE1[j] = inBytes; inBytes += al(n * sizeof(float));
        oE2[j] = inBytes; inBytes += al(n * sizeof(float));
        oS[j] = inBytes;  inBytes += al(3 * nh * sizeof(int));
        rHyp[j] = outBytes; outBytes += al(nh * sim3::kHypFloats * sizeof(float));
        rCnt[j] = outBytes; outBytes += al(nh * sizeof(int));
        rBits[j] = outBytes;
        if (inlier_bits && inlier_bits[live[j]]) outBytes += al(nh * words * sizeof(uint64_t));
    }
    std::vector<uint8_t> hin(inBytes), hout(outBytes);
    PackedTransfer P(c);
    const size_t oIn = P.add_in(hin.data(), inBytes);
    const size_t rOutBlock = P.add_out(hout.data(), outBytes);
    int rc;
    if ((rc = ensure(c, c->dPack, P.inBytes + P.outBytes + 256))) return rc;   // (upload() then finds the block large enough: the base is final)
    uint8_t *base = (uint8_t *) c->dPack.p + oIn, *obase = (uint8_t *) c->dPack.p + P.inBytes + rOutBlock;
    Sim3ProblemDev *probs = (Sim3ProblemDev *) hin.data();
    int first = 0;
    for (size_t j = 0; j < L; j++) {
        const ygzf_sim3_problem &q = p[live[j]];
        const size_t n = (size_t) q.n, nh = (size_t) q.n_hyp;
        Sim3ProblemDev &d = probs[j];
        d.X1 = (const float *) (base + oX1[j]);
        d.X2 = (const float *) (base + oX2[j]);
        d.maxErr1 = (const float *) (base + oE1[j]);
        d.maxErr2 = (const float *) (base + oE2[j]);
        d.samples = (const int *) (base + oS[j]);
        d.hyp = (float *) (obase + rHyp[j]);
        d.nInliers = (int *) (obase + rCnt[j]);
        d.bits = inlier_bits && inlier_bits[live[j]] ? (unsigned long long *) (obase + rBits[j]) : nullptr;
        d.n = q.n; d.nHyp = q.n_hyp; d.fixScale = q.fix_scale ? 1 : 0;
        d.firstHyp = first;
        first += q.n_hyp;
        memcpy(d.K1, q.K1, sizeof d.K1);
        memcpy(d.K2, q.K2, sizeof d.K2);
        memcpy(hin.data() + oX1[j], q.X3Dc1, 3 * n * sizeof(float));
        memcpy(hin.data() + oX2[j], q.X3Dc2, 3 * n * sizeof(float));
        memcpy(hin.data() + oE1[j], q.max_err1, n * sizeof(float));
        memcpy(hin.data() + oE2[j], q.max_err2, n * sizeof(float));
        memcpy(hin.data() + oS[j], q.samples, 3 * nh * sizeof(int));
    }
    uint8_t *dIn;
    if ((rc = P.upload(&dIn))) return rc;
    Sim3Args A;
    A.probs = (const Sim3ProblemDev *) (dIn + oIn);
    A.nProblems = (int) L;
    A.totalHyp = (int) totalHyp;
    launch_sim3_ransac(c->stream, A);
    HIPCHECK(c, hipGetLastError());
    if ((rc = P.download())) return rc;
    for (size_t j = 0; j < L; j++) {
        const int k = live[j];
        const size_t n = (size_t) p[k].n, nh = (size_t) p[k].n_hyp, words = (n + 63) / 64;
        memcpy(hyp[k], hout.data() + rHyp[j], nh * sim3::kHypFloats * sizeof(float));
        memcpy(n_inliers[k], hout.data() + rCnt[j], nh * sizeof(int));
        if (inlier_bits && inlier_bits[k]) memcpy(inlier_bits[k], hout.data() + rBits[j], nh * words * sizeof(uint64_t));
    }
    return YGZF_OK;
}

}  // extern "C"
