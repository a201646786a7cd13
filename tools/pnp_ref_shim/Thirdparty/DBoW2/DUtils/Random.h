// Random.h -- a scripted DUtils::Random for tools/make_golden_pnp_ref.py: RandomInt hands out the position of the case's next sample index
// in the list of still available indices, which it keeps as src/PnPsolver.cc:175-187 keeps its own (a fresh copy per iteration, each draw
// swapped with the back and popped), so that the reference's draw takes exactly that index.
#ifndef PNP_REF_RANDOM_H
#define PNP_REF_RANDOM_H
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace DUtils {
struct Random {
    static std::vector<int> &script() { static std::vector<int> s; return s; }
    static size_t &next() { static size_t n = 0; return n; }
    static int &N() { static int n = 0; return n; }
    static int &minSet() { static int n = 4; return n; }
    static std::vector<int> &avail() { static std::vector<int> a; return a; }
    static void Load(const std::vector<int> &samples, int n, int min_set) {
        script() = samples; next() = 0; N() = n; minSet() = min_set; avail().clear();
    }
    static int RandomInt(int min, int max) {
        if (next() % (size_t) minSet() == 0) {
            avail().resize(N());
            for (int i = 0; i < N(); i++) avail()[i] = i;
        }
        if (next() >= script().size()) { std::printf("the case has no sample set for iteration %zu\n", next() / minSet() + 1); std::exit(3); }
        const int want = script()[next()++];
        if (min != 0 || max != (int) avail().size() - 1) { std::printf("unexpected draw range [%d, %d]\n", min, max); std::exit(3); }
        for (int r = 0; r <= max; r++)
            if (avail()[r] == want) {
                avail()[r] = avail().back();
                avail().pop_back();
                return r;
            }
        std::printf("sample index %d is not available\n", want);
        std::exit(3);
    }
};
}  // namespace DUtils
#endif
