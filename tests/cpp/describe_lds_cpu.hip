// describe_lds_cpu.hip -- prints what csrc/describe_lds.h says about describe_window's per-wave LDS as one JSON object: row offsets, LDS-DMA
// slots, the overlay's sizes and the lane mappings of the centroid and the row blur, each with the row offset as the kernel computes it (first
// step's row + the step's constant distance).  Host code only; tests/test_describe_lds_layout.py builds it and counts bank conflicts on it.
#include <cstdio>

#include "describe_lds.h"

using namespace ygzf;

int main() {
    printf("{\"win\": %d, \"span\": %d, \"raw_bytes\": %d, \"raw_slack\": %d, \"hb_front\": %d, \"lds_bytes\": %d, \"hb_cols\": %d, \"hb_pitch\": %d,\n", kWin, kWinSpan,
           kDescRawBytes, kDescRawSlack, kHbFront, kDescLdsBytes, kHb, kHbP);
    printf(" \"row_byte\": [");
    for (int r = 0; r < kWin; r++) printf("%s%d", r ? ", " : "", desc_row_byte(r));
    printf("],\n \"slot_item\": [");   // -1: pad
    for (int s = 0; s < kDescRawSlots; s++) printf("%s%d", s ? ", " : "", desc_slot_is_pad(s) ? -1 : desc_slot_item(s));
    printf("],\n \"blur_steps\": %d, \"blur_step_rows\": %d, \"blur\": [", kDescBlurSteps, kDescBlurStepRows);   // item t = 64 * step + lane: [row, segment, row's byte offset]
    for (int t = 0; t < kDescBlurItems; t++) {
        const int s = t >> 6, lane = t & 63, r0 = desc_blur_row(lane);
        printf("%s[%d, %d, %d]", t ? ", " : "", r0 + kDescBlurStepRows * s, desc_blur_seg(lane), desc_row_byte(r0) + desc_blur_step_byte(s, r0));
    }
    printf("],\n \"centroid_steps\": %d, \"centroid\": [", kDescCenSteps);   // item 64 * step + lane: [row, dword, row's byte offset]
    for (int i = 0; i < 64 * kDescCenSteps; i++) {
        const int s = i >> 6, lane = i & 63, r0 = desc_centroid_row(0, lane);
        printf("%s[%d, %d, %d]", i ? ", " : "", r0 + kDescCenStepRows * s, desc_centroid_dword(lane), desc_row_byte(r0) + s * kDescCenStepBytes);
    }
    printf("]}\n");
    return 0;
}
