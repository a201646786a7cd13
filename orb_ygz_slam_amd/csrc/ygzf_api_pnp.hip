// ygzf_api_pnp.hip -- PnPsolver's EPnP RANSAC hypotheses and the Refine of their records, batched over solvers (C ABI of libygzf,
// include/ygzf.h; product code: no CPU fallback, nothing from oracle/ is included or linked).  The problems of one call cross the link as one
// packed upload and one packed download (ProblemBlock, ygzf_ctx.h: [records | per problem P3D P2D maxErr samples] up, [per problem hyp |
// refined hyp | counts | refined counts | refined bits] [bits] down) around the two launches of pnp_kernels.hip and one synchronisation.
#include "ygzf_ctx.h"
#include "pnp_math.h"

static_assert(YGZF_PNP_MAX_MIN_SET >= 4, "a hypothesis needs four correspondences");

extern "C" {

int ygzf_pnp_ransac(ygzf_ctx *c, int n_problems, const ygzf_pnp_problem *p, double *const *hyp, int *const *n_inliers, uint64_t *const *inlier_bits,
                    int *const *refined_n, double *const *refined_hyp, uint64_t *const *refined_bits) {
    if (!c) return YGZF_ERR_INVALID;
    if (!p || !hyp || !n_inliers || !refined_n || !refined_hyp) return fail(c, YGZF_ERR_INVALID, "null argument");
    if (n_problems <= 0) return fail(c, YGZF_ERR_INVALID, "n_problems = %d: at least one problem is needed", n_problems);
    std::vector<int> live;   // the problems with hypotheses to evaluate
    long long totalHyp = 0;
    for (int k = 0; k < n_problems; k++) {
        const ygzf_pnp_problem &q = p[k];
        if (q.n_hyp < 0) return fail(c, YGZF_ERR_INVALID, "problem %d: negative hypothesis count", k);
        if (q.n_hyp == 0) continue;
        if (q.min_set < 4 || q.min_set > YGZF_PNP_MAX_MIN_SET) return fail(c, YGZF_ERR_INVALID, "problem %d: min_set %d outside [4, %d]", k, q.min_set, YGZF_PNP_MAX_MIN_SET);
        if (q.n < q.min_set) return fail(c, YGZF_ERR_INVALID, "problem %d: %d correspondences, a hypothesis needs %d", k, q.n, q.min_set);
        if (!q.P3Dw || !q.P2D || !q.max_err || !q.samples || !hyp[k] || !n_inliers[k] || !refined_n[k] || !refined_hyp[k]) return fail(c, YGZF_ERR_INVALID, "problem %d: null array", k);
        for (int h = 0; h < q.n_hyp; h++) {
            const int *s = q.samples + (size_t) q.min_set * h;
            for (int j = 0; j < q.min_set; j++) {
                if (s[j] < 0 || s[j] >= q.n) return fail(c, YGZF_ERR_INVALID, "problem %d: hypothesis %d samples index %d outside [0, %d)", k, h, s[j], q.n);
                for (int i = 0; i < j; i++)
                    if (s[i] == s[j]) return fail(c, YGZF_ERR_INVALID, "problem %d: hypothesis %d repeats an index", k, h);
            }
        }
        live.push_back(k);
        totalHyp += q.n_hyp;
    }
    if (live.empty()) return YGZF_OK;
    if (totalHyp > (1ll << 30)) return fail(c, YGZF_ERR_INVALID, "%lld hypotheses in one call", totalHyp);
    HIPCHECK(c, hipSetDevice(c->device));
    const size_t L = live.size();
    struct Slots { ProblemBlock::Slot P3D, P2D, maxErr, samples, hyp, refHyp, counts, refN, refBits, bits; };
    std::vector<Slots> S(L);
    ProblemBlock B(c, L * sizeof(PnpProblemDev));
    bool anyBits = false;
    for (size_t j = 0; j < L; j++) {
        const int k = live[j];
        const ygzf_pnp_problem &q = p[k];
        const size_t n = (size_t) q.n, nh = (size_t) q.n_hyp, words = (n + 63) / 64;
        uint64_t *refBits = refined_bits ? refined_bits[k] : nullptr;
        S[j].P3D = B.in(q.P3Dw, 3 * n * sizeof(float));
        S[j].P2D = B.in(q.P2D, 2 * n * sizeof(float));
        S[j].maxErr = B.in(q.max_err, n * sizeof(float));
        S[j].samples = B.in(q.samples, nh * q.min_set * sizeof(int));
        S[j].hyp = B.out(hyp[k], nh * pnp::kHypDoubles * sizeof(double));
        S[j].refHyp = B.out(refined_hyp[k], nh * pnp::kHypDoubles * sizeof(double));
        S[j].counts = B.out(n_inliers[k], nh * sizeof(int));
        S[j].refN = B.out(refined_n[k], nh * sizeof(int));
        S[j].refBits = B.out(refBits, refBits ? nh * words * sizeof(uint64_t) : 0);
        if (inlier_bits && inlier_bits[k]) anyBits = true;
    }
    // The masks of the hypotheses always exist on the device (k_pnp_refine reads the records' rows).  They come last: behind the download
    // where nobody wants them, at its end -- all of them -- where somebody does.
    for (size_t j = 0; j < L; j++) {
        const ygzf_pnp_problem &q = p[live[j]];
        const size_t bytes = (size_t) q.n_hyp * (((size_t) q.n + 63) / 64) * sizeof(uint64_t);
        S[j].bits = anyBits ? B.out(inlier_bits[live[j]], bytes) : B.device_only(bytes);
    }
    int rc;
    if ((rc = B.commit())) return rc;
    PnpProblemDev *probs = B.records<PnpProblemDev>();
    int first = 0;
    for (size_t j = 0; j < L; j++) {
        const ygzf_pnp_problem &q = p[live[j]];
        PnpProblemDev &d = probs[j];
        d.P3D = B.dev<const float>(S[j].P3D);
        d.P2D = B.dev<const float>(S[j].P2D);
        d.maxErr = B.dev<const float>(S[j].maxErr);
        d.samples = B.dev<const int>(S[j].samples);
        d.hyp = B.dev<double>(S[j].hyp);
        d.refinedHyp = B.dev<double>(S[j].refHyp);
        d.nInliers = B.dev<int>(S[j].counts);
        d.refinedN = B.dev<int>(S[j].refN);
        d.refinedBits = S[j].refBits.bytes ? B.dev<uint64_t>(S[j].refBits) : nullptr;
        d.bits = B.dev<uint64_t>(S[j].bits);
        d.n = q.n; d.nHyp = q.n_hyp; d.minSet = q.min_set; d.minInliers = q.min_inliers;
        d.firstHyp = first;
        first += q.n_hyp;
        memcpy(d.K, q.K, sizeof d.K);
    }
    if ((rc = B.upload())) return rc;
    PnpArgs A;
    A.probs = B.dev_records<PnpProblemDev>();
    A.nProblems = (int) L;
    A.totalHyp = (int) totalHyp;
    launch_pnp(c->stream, A);
    HIPCHECK(c, hipGetLastError());
    return B.download();
}

}  // extern "C"
