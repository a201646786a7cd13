// tools/micro/lds_ring_read.hip -- what do fast9_quad's ring reads cost on gfx950 when the 16 ring dwords are read where they lie (ds_read_b32 at byte
// offsets 1, 2, 3: unaligned DS access is a target feature) instead of being assembled from aligned dwords with v_alignbyte_b32?
// Every wave owns a 40-row x 48-byte window (the flagship's level 7: 36 x 34 cells, nine quads per row, five rounds of the wave per cell); every lane
// plays one quad of fast9_quad's raster, 8 waves per SIMD on all CUs.  Three bodies produce the same 16 ring dwords plus the centre dword:
//   0  aligned    21 aligned reads + 14 v_alignbyte_b32 (fast9_quad as it stands)
//   1  merged     17 reads, 14 of them at byte offsets; the compiler is free to merge the dx = -2 / +2 pair of a row into one 2-byte aligned ds_read_b64
//   2  unmerged   the same 17 reads, the dx = +2 reads through a second base register, so that every read stays a ds_read_b32
// each followed by a chain of 112 v_bitop3_b32 on the results (pass 1's ratio of vector-ALU to LDS work: 32 lerps + 80 bitop3 + thresholds per quad).
// Before anything is timed, ONE workgroup writes the ring values of all three bodies to memory and the host compares them word for word; a difference
// is printed and ends the program (exit status 1) before any other launch.
// Decision rule: the byte-offset form is adopted in fast9_quad only if it takes fewer shader cycles per iteration than body 0 at 8 waves per SIMD
// (the merged form only if it is not slower than the unmerged one).
// Result (profiles/micro/r07_lds_ring_read.txt): 2202 / 9627 / 12392 shader cycles per iteration -- a ds_read_b32 off its 4-byte alignment is replayed by the
// LDS pipe (about 23 cycles of the CU's pipe per wave-read), so the aligned reads + v_alignbyte_b32 stay.
// Build + run on the GPU box:  hipcc --offload-arch=gfx950 -O3 tools/micro/lds_ring_read.hip -o /tmp/lds_ring_read && /tmp/lds_ring_read
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <vector>

constexpr int kPitch = 48, kRows = 40, kWinBytes = kRows * kPitch + 16;   // 16 bytes of slack behind the last row, as in the cell kernels
constexpr int kNq = 9, kDh = 34, kQuads = kNq * kDh, kRounds = (kQuads + 63) / 64;
constexpr int kIter = 2000, kWavesPerBlock = 4, kWords = 17;
typedef __attribute__((address_space(3))) uint8_t lds_u8;
typedef __attribute__((address_space(3), aligned(1))) unsigned lds_u32_a1;

template <int MODE>
__device__ __forceinline__ void ring_read(const uint8_t *row, unsigned (&R)[16], unsigned &centre) {   // row = byte 4q of window row y
    if (MODE == 0) {
        const unsigned *w = (const unsigned *) row;
        constexpr int pd = kPitch / 4;
#define QROW(r) const unsigned a##r = w[(r) * pd], b##r = w[(r) * pd + 1], c##r = w[(r) * pd + 2];
        QROW(0) QROW(1) QROW(2) QROW(3) QROW(4) QROW(5) QROW(6)
#undef QROW
#define AB(hi, lo, sh) __builtin_amdgcn_alignbyte(hi, lo, sh)
        R[8] = b0;             R[9] = AB(b0, a0, 3);  R[7] = AB(c0, b0, 1);
        R[10] = AB(b1, a1, 2); R[6] = AB(c1, b1, 2);
        R[11] = AB(b2, a2, 1); R[5] = AB(c2, b2, 3);
        R[12] = AB(b3, a3, 1); R[4] = AB(c3, b3, 3);
        R[13] = AB(b4, a4, 1); R[3] = AB(c4, b4, 3);
        R[14] = AB(b5, a5, 2); R[2] = AB(c5, b5, 2);
        R[0] = b6;             R[15] = AB(b6, a6, 3); R[1] = AB(c6, b6, 1);
#undef AB
        centre = b3;
    } else {
        const lds_u8 *row1 = (const lds_u8 *) row, *row2 = row1;   // LDS pointers (32 bits): a generic pointer out of the asm would be read with flat loads
        if (MODE == 2) asm volatile("" : "+v"(row2));             // a second base register: the load/store optimiser pairs reads of one base only
#define RD(p, r, dx) (*(const lds_u32_a1 *) ((p) + (r) * kPitch + 4 + (dx)))
        R[8] = RD(row1, 0, 0);   R[9] = RD(row1, 0, -1);  R[7] = RD(row1, 0, 1);
        R[10] = RD(row1, 1, -2); R[6] = RD(row2, 1, 2);
        R[11] = RD(row1, 2, -3); R[5] = RD(row1, 2, 3);
        R[12] = RD(row1, 3, -3); R[4] = RD(row1, 3, 3);
        R[13] = RD(row1, 4, -3); R[3] = RD(row1, 4, 3);
        R[14] = RD(row1, 5, -2); R[2] = RD(row2, 5, 2);
        R[0] = RD(row1, 6, 0);   R[15] = RD(row1, 6, -1); R[1] = RD(row1, 6, 1);
        centre = RD(row1, 3, 0);
#undef RD
    }
}

__device__ __forceinline__ void fill_windows(uint8_t *l, unsigned seed) {
    for (int i = threadIdx.x; i < kWavesPerBlock * kWinBytes; i += blockDim.x) l[i] = (uint8_t) ((i * 2654435761u + seed * 40503u) >> 13);
    __syncthreads();
}

// dump[(round * 64 + lane) * 17 + k] = ring dword k (k = 16: the centre) of the quad that lane plays in that round; wave 0 of one workgroup
template <int MODE>
__global__ __launch_bounds__(64 * kWavesPerBlock) void k_dump(unsigned *dump, unsigned seed) {
    __shared__ __attribute__((aligned(16))) uint8_t l[kWavesPerBlock * kWinBytes];
    fill_windows(l, seed);
    if (threadIdx.x >= 64) return;
    const int lane = threadIdx.x;
    for (int rd = 0; rd < kRounds; rd++) {
        const int i = rd * 64 + lane;
        unsigned R[16] = {}, c = 0;
        if (i < kQuads) {
            const int y = i / kNq, q = i - y * kNq;
            ring_read<MODE>(l + y * kPitch + 4 * q, R, c);
        }
        for (int k = 0; k < 16; k++) dump[i * kWords + k] = R[k];
        dump[i * kWords + 16] = c;
    }
}

template <int MODE>
__global__ __launch_bounds__(64 * kWavesPerBlock) void k_time(unsigned *out, unsigned long long *clk, unsigned seed) {
    __shared__ __attribute__((aligned(16))) uint8_t l[kWavesPerBlock * kWinBytes];
    fill_windows(l, seed);
    const int lane = threadIdx.x & 63;
    const uint8_t *win = l + (threadIdx.x >> 6) * kWinBytes;
    unsigned acc[8] = {seed, seed * 3, seed * 5, seed * 7, seed * 11, seed * 13, seed * 17, seed * 19};
    const int y0 = lane / kNq, q0 = lane - y0 * kNq, qy = 64 / kNq, qx = 64 - qy * kNq;
    int y = y0, q = q0, base = 0;
    const long long t0 = clock64();
    for (int it = 0; it < kIter; it++) {
        if (base + lane < kQuads) {
            unsigned R[16], c;
            ring_read<MODE>(win + y * kPitch + 4 * q, R, c);
            acc[0] = __builtin_amdgcn_bitop3_b32(acc[0], c, R[0], 0x96);
#pragma unroll
            for (int rep = 0; rep < 7; rep++) {
#pragma unroll
                for (int k = 0; k < 16; k++)
                    acc[k & 7] = (rep & 1) ? __builtin_amdgcn_bitop3_b32(acc[k & 7], R[k], R[(k + 1 + rep) & 15], 0xE8)
                                           : __builtin_amdgcn_bitop3_b32(acc[k & 7], R[k], R[(k + 1 + rep) & 15], 0x96);
            }
        }
        base += 64; y += qy; q += qx;
        if (q >= kNq) { q -= kNq; y++; }
        if (base >= kQuads) { base = 0; y = y0; q = q0; }
    }
    const long long t1 = clock64();
    out[blockIdx.x * blockDim.x + threadIdx.x] = acc[0] ^ acc[1] ^ acc[2] ^ acc[3] ^ acc[4] ^ acc[5] ^ acc[6] ^ acc[7];
    if (lane == 0) atomicAdd(clk, (unsigned long long) (t1 - t0));
}

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

int main() {
    hipDeviceProp_t p;
    CHECK(hipGetDeviceProperties(&p, 0));
    const int cus = p.multiProcessorCount, blocks = cus * 8;   // 4-wave workgroups, 8 per CU: 8 waves per SIMD
    printf("device %s: %d CUs; window %d rows x %d bytes per wave, %d quads in %d rounds, %d waves per SIMD\n", p.gcnArchName, cus, kRows, kPitch, kQuads,
           kRounds, 8);
    const size_t dumpWords = (size_t) kRounds * 64 * kWords;
    unsigned *out, *dump;
    unsigned long long *clk;
    CHECK(hipMalloc(&out, (size_t) blocks * 64 * kWavesPerBlock * 4));
    CHECK(hipMalloc(&dump, 3 * dumpWords * 4));
    CHECK(hipMalloc(&clk, 8));
    const char *names[3] = {"21 aligned reads + 14 v_alignbyte_b32", "17 reads at byte offsets, compiler merges", "17 reads at byte offsets, all ds_read_b32"};
    // ---- the three bodies must read the same values: one workgroup each, compared on the host before anything else is launched ----
    CHECK(hipMemset(dump, 0, 3 * dumpWords * 4));
    hipLaunchKernelGGL(k_dump<0>, dim3(1), dim3(64 * kWavesPerBlock), 0, 0, dump, 7u);
    hipLaunchKernelGGL(k_dump<1>, dim3(1), dim3(64 * kWavesPerBlock), 0, 0, dump + dumpWords, 7u);
    hipLaunchKernelGGL(k_dump<2>, dim3(1), dim3(64 * kWavesPerBlock), 0, 0, dump + 2 * dumpWords, 7u);
    CHECK(hipDeviceSynchronize());
    std::vector<unsigned> h(3 * dumpWords);
    CHECK(hipMemcpy(h.data(), dump, 3 * dumpWords * 4, hipMemcpyDeviceToHost));
    unsigned nz = 0;
    for (size_t i = 0; i < dumpWords; i++) nz |= h[i];
    if (!nz) { printf("body 0 read only zeros: the window was not filled\n"); return 1; }
    for (int m = 1; m < 3; m++)
        for (size_t i = 0; i < dumpWords; i++)
            if (h[m * dumpWords + i] != h[i]) {
                printf("DIFFERENCE body %d vs body 0: quad %zu (row %zu, quad-of-row %zu) word %zu: %08x vs %08x -- nothing else is launched\n", m, i / kWords,
                       i / kWords / kNq, i / kWords % kNq, i % kWords, h[m * dumpWords + i], h[i]);
                return 1;
            }
    printf("ring values of the three bodies are identical (%zu words each)\n", dumpWords);
    // ---- timing: shader cycles per iteration (= one quad round of the wave), mean over all waves ----
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    for (int m = 0; m < 3; m++) {
        float ms = 0;
        for (int rep = 0; rep < 2; rep++) {
            CHECK(hipMemset(clk, 0, 8));
            CHECK(hipEventRecord(e0));
            if (m == 0) hipLaunchKernelGGL(k_time<0>, dim3(blocks), dim3(64 * kWavesPerBlock), 0, 0, out, clk, 1u + rep);
            if (m == 1) hipLaunchKernelGGL(k_time<1>, dim3(blocks), dim3(64 * kWavesPerBlock), 0, 0, out, clk, 1u + rep);
            if (m == 2) hipLaunchKernelGGL(k_time<2>, dim3(blocks), dim3(64 * kWavesPerBlock), 0, 0, out, clk, 1u + rep);
            CHECK(hipEventRecord(e1));
            CHECK(hipEventSynchronize(e1));
            CHECK(hipEventElapsedTime(&ms, e0, e1));
        }
        unsigned long long c;
        CHECK(hipMemcpy(&c, clk, 8, hipMemcpyDeviceToHost));
        const double waves = (double) blocks * kWavesPerBlock;
        printf("%-44s %7.1f shader cycles per iteration per wave   (launch %.3f ms)\n", names[m], (double) c / waves / kIter, ms);
    }
    return 0;
}
