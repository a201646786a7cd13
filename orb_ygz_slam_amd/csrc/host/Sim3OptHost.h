// Sim3OptHost.h -- Optimizer::OptimizeSim3 on one host thread over csrc/sim3_opt_math.h and csrc/lm_math.h, the arithmetic k_sim3_opt compiles, with the sums in
// the reference's order (e12 then e21 of a correspondence, correspondences ascending): mode "reference" of tests/sim3_opt_cases.py bit for
// bit (tests/test_sim3_opt_host_progs.py, under -fsanitize=address,undefined).  Product code, host side, nothing of HIP, Eigen or OpenCV:
// ygz::OptimizeSim3Core runs it for calls too small to repay a launch (OptimizerSim3.cc: ygzf_host_sim3_opt_device_min), and
// tools/sim3_opt_rate.py uses it as the one-thread yardstick.
#ifndef YGZF_SIM3_OPT_HOST_H
#define YGZF_SIM3_OPT_HOST_H
#include <cmath>
#include <cstring>
#include <vector>

#include "../../../include/ygzf.h"
#include "../sim3_opt_math.h"

namespace ygz {
namespace sim3opt {

// what ygzf_optimize_sim3 returns for one problem: S12_out[8], removed[n], ret, info (may be NULL)
inline void optimize_host(const ygzf_sim3_opt_problem &c, double *S12_out, uint8_t *removed, int *ret, ygzf_sim3_opt_info *info) {
    namespace M = ygzf::sim3opt;
    namespace lm = ygzf::lm;
    const size_t n = (size_t) c.n;
    ygzf_sim3_opt_info r;
    std::memset(&r, 0, sizeof r);
    r.stop[0] = r.stop[1] = lm::kStopNotRun;
    r.n = c.n;
    std::memcpy(S12_out, c.S12, 8 * sizeof(double));
    for (size_t i = 0; i < n; i++) removed[i] = 0;
    *ret = 0;
    if (info) *info = r;
    if (c.n == 0) return;
    const M::Cam K1 = {(double) c.K1[0], (double) c.K1[1], (double) c.K1[2], (double) c.K1[3]};
    const M::Cam K2 = {(double) c.K2[0], (double) c.K2[1], (double) c.K2[2], (double) c.K2[3]};
    const double delta = (double) (float) std::sqrt((double) c.th2);   // `const float deltaHuber = sqrt(th2)`
    const double th2 = (double) c.th2;
    const bool fix = c.fix_scale != 0;
    M::S3 est, backup;
    std::memcpy(est.q, c.S12, 4 * sizeof(double));
    std::memcpy(est.t, c.S12 + 4, 3 * sizeof(double));
    est.s = c.S12[7];
    std::vector<double> chi12(n, 0.0), chi21(n, 0.0);
    lm::Lm<M::kDim, false> L;
    std::memset(&L, 0, sizeof L);
    lm::init(L);
    auto X = [](const float *v, size_t i, double o[3]) { o[0] = (double) v[3 * i]; o[1] = (double) v[3 * i + 1]; o[2] = (double) v[3 * i + 2]; };
    auto O = [](const float *v, size_t i, double o[2]) { o[0] = (double) v[2 * i]; o[1] = (double) v[2 * i + 1]; };
    for (int rnd = 0; rnd < 2; rnd++) {
        const int maxIt = rnd == 0 ? 5 : (r.n_bad > 0 ? 10 : 5);
        int reason = lm::kStopMaxIter;
        for (int it = 0; it < maxIt; it++) {
            M::S3 Tf[M::kTransforms], Ti[M::kTransforms];
            for (int j = 0; j < M::kTransforms; j++) M::so_transform(est, j, fix, Tf[j], Ti[j]);
            double acc[M::kSums];
            for (int k = 0; k < M::kSums; k++) acc[k] = 0.0;
            for (size_t i = 0; i < n; i++) {
                if (removed[i]) continue;
                double p1[3], p2[3], o1[2], o2[2];
                X(c.P1c, i, p1); X(c.P2c, i, p2); O(c.obs1, i, o1); O(c.obs2, i, o2);
                chi12[i] = M::so_edge_system(Tf, p2, K1, o1, (double) c.inv_sigma2_1[i], delta, acc);
                chi21[i] = M::so_edge_system(Ti, p1, K2, o2, (double) c.inv_sigma2_2[i], delta, acc);
            }
            lm::iteration_begin(L, acc, acc + 28, acc[35], it == 0);
            for (int trial = 0; trial < 10; trial++) {
                backup = est;
                const bool ok = lm::trial_solve(L);
                M::so_oplus(L.x, fix, est);
                M::S3 inv;
                M::so_inverse(est, inv);
                double tempChi = 0.0;
                for (size_t i = 0; i < n; i++) {
                    if (removed[i]) continue;
                    double p1[3], p2[3], o1[2], o2[2], e[2], rho0, rho1;
                    X(c.P1c, i, p1); X(c.P2c, i, p2); O(c.obs1, i, o1); O(c.obs2, i, o2);
                    M::so_error(est, p2, K1, o1, e);
                    chi12[i] = M::so_chi2(e, (double) c.inv_sigma2_1[i]);
                    lm::huber(chi12[i], delta, rho0, rho1);
                    tempChi = tempChi + rho0;
                    M::so_error(inv, p1, K2, o2, e);
                    chi21[i] = M::so_chi2(e, (double) c.inv_sigma2_2[i]);
                    lm::huber(chi21[i], delta, rho0, rho1);
                    tempChi = tempChi + rho0;
                }
                bool restore;
                const bool again = lm::trial_end(L, ok, tempChi, restore);
                if (restore) est = backup;
                if (!again) break;
            }
            r.iterations[rnd]++;
            r.trials[rnd] += L.qmax;
            const int stop = lm::iteration_end(L);
            if (stop >= 0) { reason = stop; break; }
        }
        r.stop[rnd] = reason;
        r.lambda[rnd] = L.lambda;
        r.chi2[rnd] = L.currentChi;
        int bad = 0, in = 0;
        for (size_t i = 0; i < n; i++) {
            if (removed[i]) continue;
            if (chi12[i] > th2 || chi21[i] > th2) { removed[i] = rnd == 0 ? 1 : 2; bad++; }
            else in++;
        }
        if (info) *info = r;
        if (rnd == 0) {
            r.n_bad = bad;
            if (info) *info = r;
            if (c.n - bad < 10) return;   // ret = 0 and g2oS12 is not written
        } else *ret = in;
    }
    if (info) *info = r;
    std::memcpy(S12_out, est.q, 4 * sizeof(double));
    std::memcpy(S12_out + 4, est.t, 3 * sizeof(double));
    S12_out[7] = est.s;
}

}  // namespace sim3opt
}  // namespace ygz
#endif
