// lm_host.cc -- csrc/lm_math.h, the solver k_pose_opt (N = 6) and k_sim3_opt (N = 7) share, as a plain host program: nothing of HIP.
// tests/test_lm_host_progs.py builds it with -fsanitize=address,undefined and -ffp-contract=off and holds every printed bit to the numpy
// restatement (tests/pose_opt_cases.py: ldlt, ldlt_solve; the bookkeeping as that test module restates it).
// Every double travels as the 16 hexadecimal digits of its bits, on stdin and stdout alike.
//   lm_host solve <N>     stdin: H[N N] b[N] lambda x0[N]
//                         stdout: ok | tr[N] | Hd[N N] after trial_solve | x[N] after trial_solve (x0 where the solve failed) | x[N] after an
//                         unconditional ldlt_solve of the same factor
//   lm_host script <N>    stdin: commands, one state line out per command (qmax nBadRule | lambda ni currentChi iniChi rho, then as below)
//                           begin <first> <chi2> <upper[N (N + 1) / 2]> <b[N]>   iteration_begin          + H[N N] b[N]
//                           trial <ok> <tempChi> <x[N]>                          L.x = x, then trial_end   + restore again
//                           end                                                  iteration_end            + stop
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "lm_math.h"

namespace lm = ygzf::lm;

static double rd() {
    unsigned long long u = 0;
    if (std::scanf("%llx", &u) != 1) { std::printf("short read\n"); std::exit(2); }
    const uint64_t v = (uint64_t) u;
    double d;
    std::memcpy(&d, &v, sizeof d);
    return d;
}
static void wr(double d) {
    uint64_t v;
    std::memcpy(&v, &d, sizeof v);
    std::printf(" %016llx", (unsigned long long) v);
}

template <int N> static int solve() {
    lm::Lm<N, false> L;
    std::memset(&L, 0, sizeof L);
    for (int k = 0; k < N * N; k++) L.H[k] = rd();
    for (int k = 0; k < N; k++) L.b[k] = rd();
    L.lambda = rd();
    for (int k = 0; k < N; k++) L.x[k] = rd();
    const bool ok = lm::trial_solve(L);
    std::printf("%d |", ok ? 1 : 0);
    for (int k = 0; k < N; k++) std::printf(" %d", L.tr[k]);
    std::printf(" |");
    for (int k = 0; k < N * N; k++) wr(L.Hd[k]);
    std::printf(" |");
    for (int k = 0; k < N; k++) wr(L.x[k]);
    lm::ldlt_solve(L);
    std::printf(" |");
    for (int k = 0; k < N; k++) wr(L.x[k]);
    std::printf("\n");
    return 0;
}

template <int N> static void state(const lm::Lm<N, false> &L) {
    std::printf("%d %d |", L.qmax, L.nBadRule);
    wr(L.lambda); wr(L.ni); wr(L.currentChi); wr(L.iniChi); wr(L.rho);
}

template <int N> static int script() {
    lm::Lm<N, false> L;
    std::memset(&L, 0, sizeof L);
    lm::init(L);
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "begin")) {
            int first = 0;
            if (std::scanf("%d", &first) != 1) return 2;
            const double chi2 = rd();
            double upper[N * (N + 1) / 2], b[N];
            for (int k = 0; k < N * (N + 1) / 2; k++) upper[k] = rd();
            for (int k = 0; k < N; k++) b[k] = rd();
            lm::iteration_begin(L, upper, b, chi2, first != 0);
            state(L);
            std::printf(" |");
            for (int k = 0; k < N * N; k++) wr(L.H[k]);
            for (int k = 0; k < N; k++) wr(L.b[k]);
        } else if (!std::strcmp(cmd, "trial")) {
            int ok = 0;
            if (std::scanf("%d", &ok) != 1) return 2;
            const double tempChi = rd();
            for (int k = 0; k < N; k++) L.x[k] = rd();
            bool restore = false;
            const bool again = lm::trial_end(L, ok != 0, tempChi, restore);
            state(L);
            std::printf(" | %d %d", restore ? 1 : 0, again ? 1 : 0);
        } else if (!std::strcmp(cmd, "end")) {
            const int stop = lm::iteration_end(L);
            state(L);
            std::printf(" | %d", stop);
        } else
            return 2;
        std::printf("\n");
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const int n = std::atoi(argv[2]);
    if (n != 6 && n != 7) return 2;
    if (!std::strcmp(argv[1], "solve")) return n == 6 ? solve<6>() : solve<7>();
    if (!std::strcmp(argv[1], "script")) return n == 6 ? script<6>() : script<7>();
    return 2;
}
