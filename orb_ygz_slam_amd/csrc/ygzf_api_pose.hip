// ygzf_api_pose.hip -- Optimizer::PoseOptimization(Frame *), batched over frames (C ABI of libygzf, include/ygzf.h; product code: no CPU fallback,
// nothing from oracle/ is included or linked).  The problems of one call cross the link as one packed upload and one packed download
// (ProblemBlock, ygzf_ctx.h: [records | per problem keys uRight mpValid world] up, [results | per problem flags] down) around one launch of
// k_pose_opt (pose_kernels.hip) and one synchronisation.
#include "ygzf_ctx.h"

#include <cmath>

extern "C" {

// SE3d::cast<float>(): the quaternion's coefficients converted, then normalised in float (so3.hpp:741-744)
static void pose_cast_float(const double T[7], float o[7]) {
    float q[4] = {(float) T[0], (float) T[1], (float) T[2], (float) T[3]};
    const float n = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int k = 0; k < 4; k++) o[k] = q[k] / n;
    for (int k = 4; k < 7; k++) o[k] = (float) T[k];
}

int ygzf_pose_optimization(ygzf_ctx *c, const ygzf_camera *cam, const float *inv_level_sigma2, int n_problems, const ygzf_pose_problem *p, float *Tcw_out,
                           double *Tcw_out_f64, uint8_t *const *outlier, int *ret, ygzf_pose_info *info) {
    if (!c) return YGZF_ERR_INVALID;
    if (!cam || !p || !Tcw_out || !outlier || !ret) return fail(c, YGZF_ERR_INVALID, "null argument");
    if (n_problems <= 0) return fail(c, YGZF_ERR_INVALID, "n_problems = %d: at least one problem is needed", n_problems);
    // the context's own tables have its levels; a caller's table is read up to the largest octave its correspondences name
    const int L = inv_level_sigma2 ? kMaxLevels : c->tab.cfg.nlevels;
    int maxOctave = -1;
    size_t total = 0;
    for (int k = 0; k < n_problems; k++) {
        const ygzf_pose_problem &q = p[k];
        if (q.n < 0) return fail(c, YGZF_ERR_INVALID, "problem %d: negative count", k);
        if (q.n > 0 && (!q.keys || !q.mp_valid || !q.mp_world || !outlier[k])) return fail(c, YGZF_ERR_INVALID, "problem %d: null array", k);
        for (int i = 0; i < q.n; i++) {
            if (!q.mp_valid[i]) continue;
            if (q.keys[i].octave < 0 || q.keys[i].octave >= L)
                return fail(c, YGZF_ERR_INVALID, "problem %d: keypoint %d has octave %d outside the %d levels", k, i, q.keys[i].octave, L);
            maxOctave = std::max(maxOctave, q.keys[i].octave);
        }
        total += (size_t) q.n;
    }
    HIPCHECK(c, hipSetDevice(c->device));
    int rc;
    // any n goes: the packed transfer's device block and the per-edge scratch are grow-on-demand buffers of the context (dPack, tmp.a)
    if ((rc = ensure_scratch(c, c->tmp.a, (total + 1) * sizeof(double)))) return rc;
    struct Slots { ProblemBlock::Slot keys, right, valid, world, flags; };
    std::vector<Slots> S(n_problems);
    ProblemBlock B(c, (size_t) n_problems * sizeof(PoseProblemDev), (size_t) n_problems * sizeof(PoseOut));
    for (int k = 0; k < n_problems; k++) {
        const size_t n = (size_t) p[k].n;
        S[k].keys = B.in(p[k].keys, n * sizeof(ygzf_kp));
        S[k].right = B.in(p[k].u_right, n * sizeof(float));
        S[k].valid = B.in(p[k].mp_valid, n);
        S[k].world = B.in(p[k].mp_world, n * 3 * sizeof(float));
        S[k].flags = B.out(nullptr, n);   // (merged into the caller's mvbOutlier below: only correspondences are written)
    }
    if ((rc = B.commit())) return rc;
    PoseProblemDev *probs = B.records<PoseProblemDev>();
    size_t at = 0;
    for (int k = 0; k < n_problems; k++) {
        PoseProblemDev &d = probs[k];
        d.keys = B.dev<const ygzf_kp>(S[k].keys);
        d.uRight = p[k].u_right ? B.dev<const float>(S[k].right) : nullptr;
        d.mpValid = B.dev<const uint8_t>(S[k].valid);
        d.world = B.dev<const float>(S[k].world);
        d.outlier = B.dev<uint8_t>(S[k].flags);
        d.stored = (double *) c->tmp.a.p + at;
        d.n = p[k].n;
        memcpy(d.Tcw, p[k].Tcw, sizeof d.Tcw);
        at += (size_t) p[k].n;
    }
    if ((rc = B.upload())) return rc;
    PoseArgs A;
    memset(&A, 0, sizeof A);
    A.probs = B.dev_records<PoseProblemDev>();
    A.out = B.dev_out_records<PoseOut>();
    A.fx = cam->fx; A.fy = cam->fy; A.cx = cam->cx; A.cy = cam->cy; A.bf = cam->mbf;
    A.deltaMono = (double) (float) sqrt(5.991);      // src/Optimizer.cc:1689-1690: `const float deltaMono = sqrt(5.991)`
    A.deltaStereo = (double) (float) sqrt(7.815);
    for (int l = 0; l < kMaxLevels; l++) A.invSigma2[l] = l <= maxOctave ? (inv_level_sigma2 ? inv_level_sigma2[l] : c->tab.invSigma2[l]) : 0.f;
    launch_pose_opt(c->stream, A, n_problems);
    HIPCHECK(c, hipGetLastError());
    if ((rc = B.download())) return rc;
    const PoseOut *outs = B.out_records<PoseOut>();
    for (int k = 0; k < n_problems; k++) {
        const PoseOut &o = outs[k];
        const uint8_t *flags = B.host(S[k].flags);
        ret[k] = o.ret;
        if (o.nInitial < 3) {   // src/Optimizer.cc:1767: nothing but mvbOutlier was touched
            memcpy(Tcw_out + 7 * (size_t) k, p[k].Tcw, 7 * sizeof(float));
            if (Tcw_out_f64)
                for (int j = 0; j < 7; j++) Tcw_out_f64[7 * (size_t) k + j] = (double) p[k].Tcw[j];
        } else {
            pose_cast_float(o.T, Tcw_out + 7 * (size_t) k);
            if (Tcw_out_f64) memcpy(Tcw_out_f64 + 7 * (size_t) k, o.T, 7 * sizeof(double));
        }
        for (int i = 0; i < p[k].n; i++)
            if (p[k].mp_valid[i]) outlier[k][i] = flags[i];
        if (info) {
            ygzf_pose_info &f = info[k];
            for (int r = 0; r < 4; r++) {
                f.iterations[r] = o.iters[r]; f.trials[r] = o.trials[r]; f.stop[r] = o.stop[r];
                f.lambda[r] = o.lambda[r]; f.chi2[r] = o.chi2[r];
            }
            f.n_initial = o.nInitial;
        }
    }
    return YGZF_OK;
}

}  // extern "C"
