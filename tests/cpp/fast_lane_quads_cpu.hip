// fast_lane_quads_cpu.hip -- host build of csrc/fast_lane_quads.h, the two walks that tell a lane of FAST pass 1 which quad it tests in which round,
// against the definition: in round k lane l holds quad i = 64 k + l of the cell's raster order, row i / nq, column i % nq, while i < nq * dh; the
// polarity mask is the last-quad mask in column nq - 1 and all four pixels elsewhere; the record bits are y << 2 | q << 10.
//   (no argument)   every cell of dw = 1 .. 41 by dh = 1 .. 34 tested pixels (k_fast_tab's range) and the wide cells dw = 42 .. 64 of k_fast_quads:
//                   the generic walk always, the fixed-column walk where fixed_column(nq).  Prints one JSON object with the counts and the
//                   number of mismatches; returns 1 if there is one.
//   dw dh           prints both walks of that cell, round by round, as JSON: per lane [active, y, q, mask] (the fixed walk's y and q decoded from
//                   its record bits: it does not step them), for tests/test_fast_lane_quads_cpu.py to compare with its own restatement.
// Host code only.
#include <cstdio>
#include <cstdlib>

#include "fast_lane_quads.h"

using namespace ygzf;

static int fails = 0;
#define FAIL(...)                                  \
    do {                                           \
        if (fails++ < 10) { fprintf(stderr, __VA_ARGS__); } \
    } while (0)

struct Cell {
    int dw, dh, nq, nquads, rounds;
    unsigned lastMask;
    Cell(int w, int h) : dw(w), dh(h), nq((w + 3) >> 2), nquads(nq * h), rounds((nquads + 63) >> 6), lastMask(lq::last_quad_mask(w, nq)) {}
};

// one walk of one lane, stepped as the kernel steps it
struct Stepper {
    const Cell &c;
    bool fixed;
    lq::Walk w;
    int sy, sq;
    Stepper(const Cell &cell, bool fx, int lane) : c(cell), fixed(fx) {
        if (fixed) {
            sy = 64 >> lq::log2_quads(c.nq);
            sq = 0;
            w = lq::start_fixed(lane, c.nq, c.dh, c.lastMask);
        } else {
            const unsigned m = lq::rcp16(c.nq);
            sy = lq::div_small(64, m);
            sq = 64 - sy * c.nq;
            w = lq::start_generic(lane, c.nq, m, c.dh, c.lastMask);
        }
    }
    void step() {
        if (fixed) lq::step_fixed(w, sy);
        else lq::step_generic(w, c.nq, sy, sq, c.dh, c.lastMask);
    }
    int y() const { return (int) ((w.yq >> 2) & 0xFFu); }
    int q() const { return (int) (w.yq >> 10); }
};

static long check_cell(const Cell &c, bool fixed) {
    long checked = 0;
    for (int lane = 0; lane < 64; lane++) {
        Stepper s(c, fixed, lane);
        for (int k = 0; k < c.rounds; k++, s.step()) {
            const int i = 64 * k + lane;
            const bool act = i < c.nquads;
            checked++;
            if (lq::active(s.w) != act) {
                FAIL("dw %d dh %d %s round %d lane %d: active %d, expected %d\n", c.dw, c.dh, fixed ? "fixed" : "generic", k, lane, (int) lq::active(s.w), (int) act);
                continue;
            }
            if (!act) continue;
            const int y = i / c.nq, q = i % c.nq;
            const unsigned mask = q == c.nq - 1 ? c.lastMask : lq::kAllFour;
            if (s.w.yq != (((unsigned) y << 2) | ((unsigned) q << 10)) || s.w.mask != mask || (!fixed && (s.w.y != y || s.w.q != q)))
                FAIL("dw %d dh %d %s round %d lane %d: yq %#x mask %#x, expected (%d, %d) mask %#x\n", c.dw, c.dh, fixed ? "fixed" : "generic", k, lane, s.w.yq,
                     s.w.mask, y, q, mask);
        }
    }
    return checked;
}

static void dump_walk(const Cell &c, bool fixed) {
    Stepper *s[64];
    for (int lane = 0; lane < 64; lane++) s[lane] = new Stepper(c, fixed, lane);
    printf("[");
    for (int k = 0; k < c.rounds; k++) {
        printf("%s[", k ? ", " : "");
        for (int lane = 0; lane < 64; lane++) {
            printf("%s[%d, %d, %d, %u]", lane ? ", " : "", (int) lq::active(s[lane]->w), s[lane]->y(), s[lane]->q(), s[lane]->w.mask);
            s[lane]->step();
        }
        printf("]");
    }
    printf("]");
    for (int lane = 0; lane < 64; lane++) delete s[lane];
}

int main(int argc, char **argv) {
    if (argc == 3) {
        const Cell c(atoi(argv[1]), atoi(argv[2]));
        if (c.dw < 1 || c.dw > 64 || c.dh < 1 || c.dh > 63) return 2;
        printf("{\"nq\": %d, \"rounds\": %d, \"last_mask\": %u, \"generic\": ", c.nq, c.rounds, c.lastMask);
        dump_walk(c, false);
        printf(", \"fixed\": ");
        if (lq::fixed_column(c.nq)) dump_walk(c, true);
        else printf("null");
        printf("}\n");
        return 0;
    }
    long cells = 0, fixedCells = 0, wideCells = 0, checked = 0;
    for (int dw = 1; dw <= 64; dw++)
        for (int dh = 1; dh <= 34; dh++) {
            const Cell c(dw, dh);
            (dw <= 41 ? cells : wideCells)++;
            checked += check_cell(c, false);
            if (lq::fixed_column(c.nq)) {
                if (dw <= 41) fixedCells++;
                checked += check_cell(c, true);
            }
        }
    printf("{\"cells\": %ld, \"fixed_cells\": %ld, \"wide_cells\": %ld, \"lane_rounds\": %ld, \"mismatches\": %d}\n", cells, fixedCells, wideCells, checked, fails);
    return fails ? 1 : 0;
}
