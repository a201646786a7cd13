// ygzf_api_pnp.hip -- PnPsolver's EPnP RANSAC hypotheses and the Refine of their records, batched over solvers (C ABI of libygzf,
// include/ygzf.h; product code: no CPU fallback, nothing from oracle/ is included or linked).  The problems of one call cross the link as one
// packed upload and one packed download around the two launches of pnp_kernels.hip and one synchronisation.
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
    // one host block each way, as ygzf_sim3_ransac lays its problems out: [records | per problem P3D P2D maxErr samples] up,
    // [per problem hyp | refined hyp | counts | refined counts | refined bits | bits] down.  The masks of the hypotheses always exist on the
    // device (k_pnp_refine reads the records' rows); they are the last part of the block and stay out of the download where nobody wants them.
    const size_t L = live.size();
    auto al = [](size_t b) { return (b + 63) & ~(size_t) 63; };
    std::vector<size_t> oP3(L), oP2(L), oE(L), oS(L), rHyp(L), rRef(L), rCnt(L), rRefN(L), rRefBits(L), rBits(L);
    size_t inBytes = al(L * sizeof(PnpProblemDev)), outBytes = 0;
    bool anyBits = false;
    for (size_t j = 0; j < L; j++) {
        const ygzf_pnp_problem &q = p[live[j]];
        const size_t n = (size_t) q.n, nh = (size_t) q.n_hyp, words = (n + 63) / 64;
        oP3[j] = inBytes; inBytes += al(3 * n * sizeof(float));
        oP2[j] = inBytes; inBytes += al(2 * n * sizeof(float));
        oE[j] = inBytes;  inBytes += al(n * sizeof(float));
        oS[j] = inBytes;  inBytes += al(nh * q.min_set * sizeof(int));
        rHyp[j] = outBytes; outBytes += al(nh * pnp::kHypDoubles * sizeof(double));
        rRef[j] = outBytes; outBytes += al(nh * pnp::kHypDoubles * sizeof(double));
        rCnt[j] = outBytes; outBytes += al(nh * sizeof(int));
        rRefN[j] = outBytes; outBytes += al(nh * sizeof(int));
        rRefBits[j] = outBytes;
        if (refined_bits && refined_bits[live[j]]) outBytes += al(nh * words * sizeof(uint64_t));
        if (inlier_bits && inlier_bits[live[j]]) anyBits = true;
    }
    const size_t wanted = outBytes;   // what is downloaded when no inlier_bits are wanted
    for (size_t j = 0; j < L; j++) {
        const size_t n = (size_t) p[live[j]].n, nh = (size_t) p[live[j]].n_hyp;
        rBits[j] = outBytes; outBytes += al(nh * ((n + 63) / 64) * sizeof(uint64_t));
    }
    const size_t downBytes = anyBits ? outBytes : wanted;
    std::vector<uint8_t> hin(inBytes), hout(downBytes);
    PackedTransfer P(c);
    const size_t oIn = P.add_in(hin.data(), inBytes);
    const size_t rOutBlock = P.add_out(hout.data(), downBytes);
    int rc;
    if ((rc = ensure(c, c->dPack, P.inBytes + PackedTransfer::al(outBytes) + 512))) return rc;   // (upload() then finds the block large enough: the base is final)
    uint8_t *base = (uint8_t *) c->dPack.p + oIn, *obase = (uint8_t *) c->dPack.p + P.inBytes + rOutBlock;
    PnpProblemDev *probs = (PnpProblemDev *) hin.data();
    int first = 0;
    for (size_t j = 0; j < L; j++) {
        const ygzf_pnp_problem &q = p[live[j]];
        const size_t n = (size_t) q.n, nh = (size_t) q.n_hyp;
        PnpProblemDev &d = probs[j];
        d.P3D = (const float *) (base + oP3[j]);
        d.P2D = (const float *) (base + oP2[j]);
        d.maxErr = (const float *) (base + oE[j]);
        d.samples = (const int *) (base + oS[j]);
        d.hyp = (double *) (obase + rHyp[j]);
        d.refinedHyp = (double *) (obase + rRef[j]);
        d.nInliers = (int *) (obase + rCnt[j]);
        d.refinedN = (int *) (obase + rRefN[j]);
        d.refinedBits = refined_bits && refined_bits[live[j]] ? (uint64_t *) (obase + rRefBits[j]) : nullptr;
        d.bits = (uint64_t *) (obase + rBits[j]);
        d.n = q.n; d.nHyp = q.n_hyp; d.minSet = q.min_set; d.minInliers = q.min_inliers;
        d.firstHyp = first;
        first += q.n_hyp;
        memcpy(d.K, q.K, sizeof d.K);
        memcpy(hin.data() + oP3[j], q.P3Dw, 3 * n * sizeof(float));
        memcpy(hin.data() + oP2[j], q.P2D, 2 * n * sizeof(float));
        memcpy(hin.data() + oE[j], q.max_err, n * sizeof(float));
        memcpy(hin.data() + oS[j], q.samples, nh * q.min_set * sizeof(int));
    }
    uint8_t *dIn;
    if ((rc = P.upload(&dIn))) return rc;
    PnpArgs A;
    A.probs = (const PnpProblemDev *) (dIn + oIn);
    A.nProblems = (int) L;
    A.totalHyp = (int) totalHyp;
    launch_pnp(c->stream, A);
    HIPCHECK(c, hipGetLastError());
    if ((rc = P.download())) return rc;
    for (size_t j = 0; j < L; j++) {
        const int k = live[j];
        const size_t n = (size_t) p[k].n, nh = (size_t) p[k].n_hyp, words = (n + 63) / 64;
        memcpy(hyp[k], hout.data() + rHyp[j], nh * pnp::kHypDoubles * sizeof(double));
        memcpy(refined_hyp[k], hout.data() + rRef[j], nh * pnp::kHypDoubles * sizeof(double));
        memcpy(n_inliers[k], hout.data() + rCnt[j], nh * sizeof(int));
        memcpy(refined_n[k], hout.data() + rRefN[j], nh * sizeof(int));
        if (refined_bits && refined_bits[k]) memcpy(refined_bits[k], hout.data() + rRefBits[j], nh * words * sizeof(uint64_t));
        if (inlier_bits && inlier_bits[k]) memcpy(inlier_bits[k], hout.data() + rBits[j], nh * words * sizeof(uint64_t));
    }
    return YGZF_OK;
}

}  // extern "C"
