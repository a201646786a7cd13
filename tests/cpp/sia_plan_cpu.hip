// sia_plan_cpu.hip -- what csrc/lds_layout.h decides for one-pair SparseImgAlign launches (ygzf_sia_run: capBytes = 0), as a stand-alone host
// program: the plan of sia_lds() at the kernel's ceiling and, per level, k_sia_run's own test "imgBytes + 8 <= stageBytes".
//   sia_plan_cpu <static LDS bytes, 0: the bound below> <features>:<bytes of level>,<bytes of level>,... ...
// prints a JSON list, one record per launch.  The static LDS is a constant of the compiled kernel (hipFuncGetAttributes); without a device the
// bound read off k_sia_run's declarations stands in: s_red[(512 / 16) * 30], s_tot[30], s_H[36], two floats, three Se3 (seven floats) and four
// ints.  The ceiling is counted in allocation units of 256 bytes, so any value in (4096, 4352] gives the same one.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "lds_layout.h"

using namespace ygzf;

constexpr size_t kSiaStaticBound = sizeof(float) * ((512 / 16) * 30 + 30 + 36 + 2 + 3 * 7) + sizeof(int) * 4;

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: sia_plan_cpu <static LDS bytes | 0> <features>:<level bytes>,... ...\n");
        return 2;
    }
    const size_t stat = atoi(argv[1]) > 0 ? (size_t) atoi(argv[1]) : kSiaStaticBound;
    const int ceiling = sia_ceiling(stat);
    printf("[");
    for (int a = 2; a < argc; a++) {
        char *p = argv[a];
        const int n = (int) strtol(p, &p, 10);
        if (*p != ':') return 2;
        size_t bytes[16], largest = 0;
        int nl = 0;
        while (*p && nl < 16) {
            p++;
            bytes[nl] = (size_t) strtoll(p, &p, 10);
            if (bytes[nl] > largest) largest = bytes[nl];
            nl++;
        }
        const SiaLds L = sia_lds(n, largest, (size_t) ceiling, 0);
        printf("%s{\"features\": %d, \"static\": %zu, \"ceiling\": %d, \"fits\": %d, \"jac\": %d, \"stage_off\": %d, \"stage_bytes\": %d, \"total\": %zu, \"staged\": [", a > 2 ? ", " : "", n, stat,
               ceiling, sia_fits(L) ? 1 : 0, L.jac, L.stageOff, L.stageBytes, sia_lds_bytes(L));
        for (int l = 0; l < nl; l++) printf("%s%d", l ? ", " : "", bytes[l] + 8 <= (size_t) L.stageBytes ? 1 : 0);
        printf("]}");
        if (sia_fits(L) && sia_lds_bytes(L) > (size_t) ceiling) {
            fprintf(stderr, "FAILED: %d features: %zu bytes above the ceiling %d\n", n, sia_lds_bytes(L), ceiling);
            return 1;
        }
    }
    printf("]\n");
    return 0;
}
