// describe_lds.h -- the per-wave LDS of describe_window (csrc/extract_kernels.hip): where every row of the raw 43 x 43 window lies, which 16-byte
// LDS-DMA slot carries which piece of it, how the row-blurred window shares the memory, which lane takes which work item of the two
// phases that read the raw window, and where the column pass keeps its sampled bytes.  Plain constexpr arithmetic, no device code: the kernel
// computes its addresses with these functions and tests/cpp/describe_lds_cpu.hip prints them for tests/test_describe_lds_layout.py, which
// counts the bank conflicts they give (the column pass's: tools/describe_column_banks.py, tests/test_describe_column_order.py).
//
// The bank rule the layout answers (gfx950): a ds_read_b32 is served in two groups of 32 lanes, the bank of byte address a is (a / 4) mod 32,
// and every further distinct dword on a bank costs the group one more cycle.  Rows 64 bytes apart start on banks 0, 16, 0, 16, ...: in the row
// blur a group of 32 lanes holds 8 consecutive rows x 4 segments, so four of its rows share every bank (3.67-way on average), and the
// centroid's 4 rows x 8 dwords are 2-way.  Here every second row is followed by one unused 16-byte slot: row pairs lie 144 bytes = 36 dwords
// apart and the 8 rows of a blur group start on banks 4k + {0, 16, 4, 20, 8, 24, 12, 28}.  With every row at the same offset inside its span
// (row pitch a multiple of 16) the blur's reads are conflict-free where the window starts 0 or 1 bytes past a dword and 2-way otherwise -- its
// segments then start 0, 3, 5 and 8 dwords into the row, and 8 meets another row's 0 --, and the centroid, whose groups take rows
// {r, r + 1, r + 4, r + 5}, is conflict-free.
#ifndef YGZF_DESCRIBE_LDS_H
#define YGZF_DESCRIBE_LDS_H

namespace ygzf {

constexpr int kWin = 43;            // raw window: 43 rows (ky - 21 .. ky + 21) of 43 bytes, each inside a 16-byte aligned span of kWinSpan bytes
constexpr int kWinSpan = 64;
constexpr int kHb = 37, kHbP = 40;  // row-blurred window: 43 rows x 37 columns (u16), pitch even for 32-bit stores

// The pad slots.  The LDS-DMA fills 64 slots per instruction, so three instructions carry 192 slots = 43 x 4 + 20: one of the 21 gaps between
// row pairs has no pad.  It is the one after row 39, where a blur group (rows 32 .. 39) ends and past the last row the centroid reads (37):
// rows 38 .. 41 are contiguous, every lane group still sees the bank pattern above, and only rows 40 .. 42 lie 16 bytes lower than the rule
// "one slot after every second row" puts them.
constexpr int kDescNoPadAfter = 39;
constexpr int desc_pads_before(int r) { return (r >> 1) - (r > kDescNoPadAfter ? 1 : 0); }
// byte offset of window row r's span inside the raw region
constexpr int desc_row_byte(int r) { return kWinSpan * r + 16 * desc_pads_before(r); }
constexpr int kDescRawSlots = desc_row_byte(kWin - 1) / 16 + kWinSpan / 16;   // 192
constexpr int kDescRawSlack = 16;
constexpr int kDescRawBytes = 16 * kDescRawSlots + kDescRawSlack;             // 3088

// What LDS-DMA slot s (bytes 16 s .. 16 s + 15 of the raw region) holds: a pad, whose lane loads nothing, or item 4 * row + quarter of the
// row's span.  Slots 0 .. 170 are 19 runs of two rows and a pad, 171 .. 186 rows 38 .. 41, 187 the last pad, 188 .. 191 row 42.
constexpr int kDescRunSlots = 2 * kWinSpan / 16 + 1;                          // 9
constexpr int kDescRegularSlots = kDescRunSlots * ((kDescNoPadAfter - 1) / 2);   // 171
constexpr int kDescLastPadSlot = desc_row_byte(kWin - 1) / 16 - 1;            // 187
constexpr bool desc_slot_is_pad(int s) { return s < kDescRegularSlots ? s % kDescRunSlots == kDescRunSlots - 1 : s == kDescLastPadSlot; }
constexpr int desc_slot_item(int s) {   // of a slot that is no pad
    return s - (s < kDescRegularSlots ? s / kDescRunSlots : kDescRegularSlots / kDescRunSlots) - (s > kDescLastPadSlot ? 1 : 0);
}
constexpr bool desc_slots_ok() {   // every quarter of every row has exactly the slot desc_row_byte gives it
    int next = 0;
    for (int s = 0; s < kDescRawSlots; s++) {
        if (desc_slot_is_pad(s)) continue;
        if (desc_slot_item(s) != next || 16 * s != desc_row_byte(next >> 2) + 16 * (next & 3)) return false;
        next++;
    }
    return next == kWin * 4;
}
static_assert(desc_slots_ok(), "LDS-DMA slots and row offsets disagree");
// The same for the three slots 64 p + lane of one lane, from ONE division: 64 p = 9 * 7 p + p, so slot 64 p + lane lies in run 7 p + (lane + p) / 9 at
// place (lane + p) % 9.  With run0 = lane / 9 and k0 = lane % 9 the later pieces' runs are 7 p + run0 + (k0 >= 9 - p) and their pads the lanes with
// k0 = 8 - p: a compare each instead of a division and a remainder each.
struct DescLaneSlots { int item[kDescRawSlots / 64]; bool pad[kDescRawSlots / 64]; };   // (a pad's item is not meant)
constexpr DescLaneSlots desc_lane_slots(int lane) {
    DescLaneSlots d{};
    const int run0 = lane / kDescRunSlots, k0 = lane - kDescRunSlots * run0;
    for (int p = 0; p < kDescRawSlots / 64; p++) {
        const int s = 64 * p + lane;
        const int run = (64 / kDescRunSlots) * p + run0 + (k0 >= kDescRunSlots - p ? 1 : 0);
        const bool regular = 64 * (p + 1) <= kDescRegularSlots || s < kDescRegularSlots;
        d.item[p] = s - (regular ? run : kDescRegularSlots / kDescRunSlots) - (s > kDescLastPadSlot ? 1 : 0);
        d.pad[p] = regular ? k0 == kDescRunSlots - 1 - p : s == kDescLastPadSlot;
    }
    return d;
}
constexpr bool desc_lane_slots_ok() {
    for (int lane = 0; lane < 64; lane++)
        for (int p = 0; p < kDescRawSlots / 64; p++) {
            const DescLaneSlots d = desc_lane_slots(lane);
            if (d.pad[p] != desc_slot_is_pad(64 * p + lane) || (!d.pad[p] && d.item[p] != desc_slot_item(64 * p + lane))) return false;
        }
    return true;
}
static_assert(64 % kDescRunSlots == 1 && desc_lane_slots_ok(), "a lane's three slots from one division disagree with desc_slot_item");

// ---- lane mappings of the phases that read the raw window ------------------------------------------------------------------------------------
// Row blur: 43 rows x 4 segments of 10 columns = 172 items, item t = 64 * step + lane -> row t >> 2, segment t & 3 (three steps, the third
// with 44 lanes).  Later steps of a lane are 16 rows further down.
constexpr int kDescBlurItems = kWin * 4, kDescBlurSteps = 3, kDescBlurStepRows = 16;
constexpr int desc_blur_row(int t) { return t >> 2; }
constexpr int desc_blur_seg(int t) { return t & 3; }
// Centroid: rows 6 .. 37 (v = -15 .. 16, the last one empty) x 8 dwords = 256 items in four steps of 8 rows.  A group of 32 lanes takes
// rows {R, R + 1, R + 4, R + 5} (lanes 0 .. 31) or {R + 2, R + 3, R + 6, R + 7} (lanes 32 .. 63) of its step: four rows whose spans start
// 8 banks apart, each read over 8 consecutive dwords.
constexpr int kDescCenRow0 = 6, kDescCenSteps = 4, kDescCenStepRows = 8;
constexpr int desc_centroid_row(int step, int lane) {
    return kDescCenRow0 + kDescCenStepRows * step + 2 * (lane >> 5) + ((lane >> 3) & 1) + 4 * ((lane >> 4) & 1);
}
constexpr int desc_centroid_dword(int lane) { return lane & 7; }

// A lane's later steps lie a constant number of bytes past its first one, so the kernel computes one address per phase and the steps become
// instruction offsets: the centroid's rows (all above the missing pad) 576 bytes per step, the blur's 1152, less 16 below the missing pad.
// (The offset inside the span repeats as well: row pitches are multiples of 4 on this path, so 8 rows x (pitch & 15) is a multiple of 16.)
constexpr int kDescCenStepBytes = desc_row_byte(kDescCenRow0 + kDescCenStepRows) - desc_row_byte(kDescCenRow0);
constexpr int kDescBlurStepBytes = desc_row_byte(kDescBlurStepRows) - desc_row_byte(0);
constexpr int desc_blur_step_byte(int step, int row0) {   // from row0 < 16 to row0 + 16 * step
    return step * kDescBlurStepBytes - (row0 + kDescBlurStepRows * step > kDescNoPadAfter ? 16 : 0);
}
constexpr bool desc_steps_ok() {
    for (int lane = 0; lane < 64; lane++)
        for (int s = 0; s < kDescCenSteps; s++)
            if (desc_row_byte(desc_centroid_row(s, lane)) != desc_row_byte(desc_centroid_row(0, lane)) + s * kDescCenStepBytes) return false;
    for (int t = 0; t < kDescBlurItems; t++) {
        const int s = t >> 6, r0 = desc_blur_row(t & 63);
        if (desc_blur_row(t) != r0 + kDescBlurStepRows * s || desc_blur_seg(t) != desc_blur_seg(t & 63)) return false;
        if (desc_row_byte(desc_blur_row(t)) != desc_row_byte(r0) + desc_blur_step_byte(s, r0)) return false;
    }
    return true;
}
static_assert(desc_steps_ok(), "a lane's steps are not the constant distances apart that the kernel adds");

// ---- the overlay ------------------------------------------------------------------------------------------------------------------------------
// hb (43 rows x 40 u16 = 3440 bytes) starts at the wave's first byte, the raw region kHbFront bytes in.  The centroid is taken before the blur
// writes anything; blur step s reads raw rows 16 s .. 16 s + 15 and then writes hb rows 16 s .. 16 s + 15, and a wave's LDS operations execute
// in order.  So hb's rows of step s may lie over raw rows of EARLIER steps only (rows < 16 s), and step 0's over none:
//     80 * 16 * (s + 1) <= kHbFront + desc_row_byte(16 * s)   for s = 0, 1   (1280 <= front; 2560 <= front + 1152)
//     80 * 43           <= kHbFront + desc_row_byte(32)       for s = 2      (3440 <= front + 2304)
// -> kHbFront >= 1408.  Per wave that is 1408 + 3088 = 4496 bytes; at most 5120 (160 KB / 32 wave slots) keeps LDS from limiting the CU's occupancy.
constexpr int kHbBytes = kWin * kHbP * 2;
constexpr int kHbFront = 1408;
constexpr int kDescLdsBytes = kHbFront + kDescRawBytes;
constexpr bool desc_overlay_ok(int front) {
    for (int s = 0; s < kDescBlurSteps; s++) {
        const int rowsEnd = kDescBlurStepRows * (s + 1) < kWin ? kDescBlurStepRows * (s + 1) : kWin;
        if (rowsEnd * kHbP * 2 > front + (s ? desc_row_byte(kDescBlurStepRows * s) : 0)) return false;
    }
    return true;
}
static_assert(desc_overlay_ok(kHbFront) && !desc_overlay_ok(kHbFront - 16), "hb overlays raw rows that are still to be read (or the front is larger than needed)");
static_assert(kHbFront % 16 == 0 && kDescLdsBytes % 16 == 0 && kHbBytes <= kDescLdsBytes && kDescLdsBytes <= 5120, "per-wave LDS of k_describe");
static_assert(kDescRawSlots == 3 * 64, "three LDS-DMA instructions carry the raw window");

// ---- the column pass ----------------------------------------------------------------------------------------------------------------------------
// The column blur is taken only at the pattern's rotated points, each distinct point once: lane l of sample step s holds point 64 s + l of
// kBriefPoint (orb_pattern_table.h: tile order, so that a group of 32 lanes reads a compact cluster of hb -- neighbouring columns share a dword,
// neighbouring rows lie kHbP / 2 = 20 banks apart; tools/describe_column_banks.py counts the cycles) and stores the blurred byte at val[64 s + l];
// the pairs then compare two bytes of val.  val lies right behind hb, over raw rows that are dead once the row blur has run.
constexpr int kDescSampleSteps = 6, kDescValBytes = 64 * kDescSampleSteps;
constexpr int kDescValByte = 3440;
static_assert(kDescValByte >= kHbBytes && kDescValByte % 4 == 0 && kDescValByte + kDescValBytes <= kDescLdsBytes, "val lies behind hb, inside the wave's LDS");

}  // namespace ygzf
#endif
