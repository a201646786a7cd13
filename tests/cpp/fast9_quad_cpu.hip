// fast9_quad_cpu.hip -- host build of csrc/fast9_quad.h (the thresholds, comparison and arc network of fast9_quad) checked against the definitions:
//   arcs        every 16-bit ring mask in bit 7 of each of the four byte lanes, random low bits: bright <=> nine contiguous ones of the circular
//               sixteen, not-dark <=> no nine contiguous zeros
//   thresholds  every centre x every ring value x t in {0, 1, 5, 7, 20, 40, 127, 128, 130, 254, 255} x the four byte positions of a dword, other
//               values in the other three: bright bit <=> ring > c + t, not-dark bit <=> ring >= c - t
//   whole       100 000 random quads from full-range values and 100 000 from {0, 3, 252, 255} against the scalar FAST 9/16 rule
// Host code only; tests/test_fast9_quad_cpu.py builds it (with the sanitizers) and runs it.  Prints "fast9 quad ok" and returns 0, or the first
// mismatches and 1.
#include <cstdint>
#include <cstdio>

#include "fast9_quad.h"

using namespace ygzf;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd() {   // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (unsigned) ((z ^ (z >> 31)) >> 16);
}

static int fails = 0;
#define FAIL(...)                                  \
    do {                                           \
        if (fails++ < 10) { printf(__VA_ARGS__); } \
    } while (0)

// the definition: nine contiguous set bits in the circular 16-bit mask
static bool arc9(unsigned m) {
    for (int s = 0; s < 16; s++) {
        int n = 0;
        while (n < 9 && ((m >> ((s + n) & 15)) & 1u)) n++;
        if (n == 9) return true;
    }
    return false;
}

// scalar FAST 9/16 at threshold t: 1 bright, 2 dark, 0 none
static unsigned scalar_pol(int c, const int *ring, int t) {
    unsigned mb = 0, md = 0;
    for (int k = 0; k < 16; k++) {
        if (ring[k] > c + t) mb |= 1u << k;
        if (ring[k] < c - t) md |= 1u << k;
    }
    return arc9(mb) ? 1u : (arc9(md) ? 2u : 0u);
}

static void check_arcs() {
    static bool want[65536];
    for (unsigned m = 0; m < 65536; m++) want[m] = arc9(m);
    // four masks per step, one per byte lane: lane j holds mask (m + 16411 * j) mod 65536, so every lane sees every mask
    for (unsigned m = 0; m < 65536; m++) {
        unsigned mk[4], B[16];
        for (int j = 0; j < 4; j++) mk[j] = (m + 16411u * j) & 0xFFFFu;
        for (int k = 0; k < 16; k++) {
            B[k] = rnd() & 0x7F7F7F7Fu;
            for (int j = 0; j < 4; j++) B[k] |= ((mk[j] >> k) & 1u) << (8 * j + 7);
        }
        const unsigned br = f9::arcs_bright(B), nd = f9::arcs_not_dark(B);
        for (int j = 0; j < 4; j++) {
            const bool gb = (br >> (8 * j + 7)) & 1u, gn = (nd >> (8 * j + 7)) & 1u;
            if (gb != want[mk[j]]) FAIL("arcs_bright: mask %04x lane %d gives %d\n", mk[j], j, (int) gb);
            if (gn != !want[~mk[j] & 0xFFFFu]) FAIL("arcs_not_dark: mask %04x lane %d gives %d\n", mk[j], j, (int) gn);   // dark = nine contiguous zeros
        }
    }
}

static void check_thresholds() {
    const int ts[] = {0, 1, 5, 7, 20, 40, 127, 128, 130, 254, 255};
    for (int t : ts)
        for (int pos = 0; pos < 4; pos++)
            for (unsigned c = 0; c < 256; c++) {
                // the other three bytes: values that differ from c and from each other
                unsigned centre = 0;
                for (int j = 0; j < 4; j++) centre |= (j == pos ? c : ((c * 7u + 83u * (unsigned) j + 41u) & 0xFFu)) << (8 * j);
                const f9::Thresholds th = f9::thresholds(centre, t);
                for (unsigned r = 0; r < 256; r++) {
                    unsigned ring = 0;
                    for (int j = 0; j < 4; j++) ring |= (j == pos ? r : ((r * 5u + 59u * (unsigned) j + 17u) & 0xFFu)) << (8 * j);
                    const unsigned B = f9::lerp_u8(ring, th.nhi, 0u), N = f9::lerp_u8(ring, th.nlo, 0x01010101u);
                    for (int j = 0; j < 4; j++) {
                        const int cj = (int) ((centre >> (8 * j)) & 0xFFu), rj = (int) ((ring >> (8 * j)) & 0xFFu);
                        const bool gb = (B >> (8 * j + 7)) & 1u, gn = (N >> (8 * j + 7)) & 1u;
                        if (gb != (rj > cj + t)) FAIL("bright: c %d ring %d t %d byte %d gives %d\n", cj, rj, t, j, (int) gb);
                        if (gn != (rj >= cj - t)) FAIL("not dark: c %d ring %d t %d byte %d gives %d\n", cj, rj, t, j, (int) gn);
                    }
                }
            }
}

static void check_whole(bool extremes, int n) {
    static const int ext[4] = {0, 3, 252, 255};
    const int ts[] = {7, 20, 5, 40, 0, 1, 127, 250, 255};
    int seen[3] = {0, 0, 0};
    for (int it = 0; it < n; it++) {
        int c[4], ring[4][16];
        unsigned centre = 0, R[16] = {0};
        for (int j = 0; j < 4; j++) {
            c[j] = extremes ? ext[rnd() & 3u] : (int) (rnd() & 0xFFu);
            centre |= (unsigned) c[j] << (8 * j);
            // full-range quads: half of them with ring values near the centre, so that arcs around the threshold occur
            const bool near = !extremes && (rnd() & 1u);
            for (int k = 0; k < 16; k++) {
                int v = extremes ? ext[rnd() & 3u] : (int) (rnd() & 0xFFu);
                if (near) { v = c[j] + (int) (rnd() % 61u) - 30; v = v < 0 ? 0 : (v > 255 ? 255 : v); }
                ring[j][k] = v;
                R[k] |= (unsigned) v << (8 * j);
            }
        }
        const int t = ts[it % (int) (sizeof ts / sizeof ts[0])];
        const unsigned got = f9::polarity(R, f9::thresholds(centre, t));
        for (int j = 0; j < 4; j++) {
            const unsigned w = scalar_pol(c[j], ring[j], t), g = (got >> (8 * j)) & 0xFFu;
            seen[w]++;
            if (g != w) FAIL("whole (%s): quad %d byte %d t %d centre %d gives %u, the rule %u\n", extremes ? "extremes" : "full range", it, j, t, c[j], g, w);
        }
    }
    printf("whole (%s): %d none, %d bright, %d dark by the rule\n", extremes ? "extremes" : "full range", seen[0], seen[1], seen[2]);
    if (seen[1] < 100 || seen[2] < 100) FAIL("whole (%s): the draw holds too few corners to mean anything\n", extremes ? "extremes" : "full range");
}

int main() {
    check_arcs();
    check_thresholds();
    check_whole(false, 100000);
    check_whole(true, 100000);
    if (fails) {
        printf("fast9 quad: %d mismatches\n", fails);
        return 1;
    }
    printf("fast9 quad ok\n");
    return 0;
}
