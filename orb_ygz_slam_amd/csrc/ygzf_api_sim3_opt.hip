// ygzf_api_sim3_opt.hip -- Optimizer::OptimizeSim3, batched over loop candidates (C ABI of libygzf, include/ygzf.h; product code: no CPU
// fallback, nothing from oracle/ is included or linked).  The problems of one call cross the link as one packed upload and one packed download
// (ProblemBlock, ygzf_ctx.h: [records | per problem one segment of floats] up, [results | per problem flags] down) around one launch of
// k_sim3_opt (sim3_opt_kernels.hip) and one synchronisation.
#include "ygzf_ctx.h"

#include <cmath>

extern "C" {

int ygzf_optimize_sim3(ygzf_ctx *c, int n_problems, const ygzf_sim3_opt_problem *p, double *S12_out, uint8_t *const *removed, int *ret,
                       ygzf_sim3_opt_info *info) {
    if (!c) return YGZF_ERR_INVALID;
    if (!p || !S12_out || !removed || !ret) return fail(c, YGZF_ERR_INVALID, "null argument");
    if (n_problems <= 0) return fail(c, YGZF_ERR_INVALID, "n_problems = %d: at least one problem is needed", n_problems);
    size_t total = 0;
    for (int k = 0; k < n_problems; k++) {
        const ygzf_sim3_opt_problem &q = p[k];
        if (q.n < 0) return fail(c, YGZF_ERR_INVALID, "problem %d: negative count", k);
        if (q.n > 0 && (!q.P1c || !q.P2c || !q.obs1 || !q.obs2 || !q.inv_sigma2_1 || !q.inv_sigma2_2 || !removed[k]))
            return fail(c, YGZF_ERR_INVALID, "problem %d: null array", k);
        total += (size_t) q.n;
    }
    HIPCHECK(c, hipSetDevice(c->device));
    int rc;
    // any n goes: the packed transfer's device block and the per-edge scratch are grow-on-demand buffers of the context (dPack, tmp.a)
    if ((rc = ensure_scratch(c, c->tmp.a, (2 * total + 1) * sizeof(double)))) return rc;
    // per problem one segment of floats: P1c[3n] P2c[3n] obs1[2n] obs2[2n] inv_sigma2_1[n] inv_sigma2_2[n]
    struct Slots { ProblemBlock::Slot seg, flags; };
    std::vector<Slots> S(n_problems);
    ProblemBlock B(c, (size_t) n_problems * sizeof(Sim3OptProblemDev), (size_t) n_problems * sizeof(Sim3OptOut));
    for (int k = 0; k < n_problems; k++) {
        S[k].seg = B.in_own(12 * (size_t) p[k].n * sizeof(float));
        S[k].flags = B.out(removed[k], (size_t) p[k].n);
    }
    if ((rc = B.commit())) return rc;
    Sim3OptProblemDev *probs = B.records<Sim3OptProblemDev>();
    size_t at = 0;
    for (int k = 0; k < n_problems; k++) {
        const ygzf_sim3_opt_problem &q = p[k];
        const size_t n = (size_t) q.n;
        Sim3OptProblemDev &d = probs[k];
        const float *seg = B.dev<const float>(S[k].seg);
        float *h = (float *) B.host(S[k].seg);
        d.P1c = seg;               d.P2c = seg + 3 * n;
        d.obs1 = seg + 6 * n;      d.obs2 = seg + 8 * n;
        d.invSigma2_1 = seg + 10 * n; d.invSigma2_2 = seg + 11 * n;
        d.removed = B.dev<uint8_t>(S[k].flags);
        d.stored = (double *) c->tmp.a.p + 2 * at;
        d.n = q.n;
        d.fixScale = q.fix_scale ? 1 : 0;
        for (int j = 0; j < 4; j++) { d.K1[j] = (double) q.K1[j]; d.K2[j] = (double) q.K2[j]; }
        memcpy(d.S12, q.S12, sizeof d.S12);
        d.th2 = (double) q.th2;
        d.delta = (double) (float) sqrt((double) q.th2);   // src/Optimizer.cc:2458: `const float deltaHuber = sqrt(th2)`
        if (n) {
            memcpy(h, q.P1c, 3 * n * sizeof(float));           memcpy(h + 3 * n, q.P2c, 3 * n * sizeof(float));
            memcpy(h + 6 * n, q.obs1, 2 * n * sizeof(float));  memcpy(h + 8 * n, q.obs2, 2 * n * sizeof(float));
            memcpy(h + 10 * n, q.inv_sigma2_1, n * sizeof(float)); memcpy(h + 11 * n, q.inv_sigma2_2, n * sizeof(float));
        }
        at += n;
    }
    if ((rc = B.upload())) return rc;
    Sim3OptArgs A;
    A.probs = B.dev_records<Sim3OptProblemDev>();
    A.out = B.dev_out_records<Sim3OptOut>();
    launch_sim3_opt(c->stream, A, n_problems);
    HIPCHECK(c, hipGetLastError());
    if ((rc = B.download())) return rc;
    const Sim3OptOut *outs = B.out_records<Sim3OptOut>();
    for (int k = 0; k < n_problems; k++) {
        const Sim3OptOut &o = outs[k];
        ret[k] = o.ret;
        memcpy(S12_out + 8 * (size_t) k, o.S, 8 * sizeof(double));   // (S12 itself, bit for bit, where g2oS12 is not written)
        if (info) {
            ygzf_sim3_opt_info &f = info[k];
            for (int r = 0; r < 2; r++) {
                f.iterations[r] = o.iters[r]; f.trials[r] = o.trials[r]; f.stop[r] = o.stop[r];
                f.lambda[r] = o.lambda[r]; f.chi2[r] = o.chi2[r];
            }
            f.n = p[k].n;
            f.n_bad = o.nBad;
        }
    }
    return YGZF_OK;
}

}  // extern "C"
