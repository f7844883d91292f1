// ccsx_scan.hip -- MI355X (gfx950) kernel of the adapter scanner (SPEC.md §17):
// every pattern of the adapter set (each adapter and its reverse complement)
// against every column of whole CCS reads, and every (read, pattern, column)
// whose bottom row reaches the pattern's threshold.  host/scan.cpp is the same
// definition as a sequential loop.
//
// The mapping is ccsx_barcode.hip's turned round.  There a lane owns a pattern
// and the text is wave-uniform; here the pattern is wave-uniform (its two bit
// planes, row mask, length and threshold are scalar loads of an outer loop over
// the set) and a lane owns a tile of one read: the columns [t0, t0 + kTC).  The
// lane keeps the column H(1 .. LR, j) in LR VGPRs, builds the column's match
// mask from its own base (three bitwise operations per plane on a 64-bit
// pair), and a cell is its match bit, one multiply-add, a max3 and the penalty.
// Patterns shorter than LR are right-aligned (ccsx_scan.h); a pattern of LR
// bases runs the body without the per-row test (wave-uniform branch).
//
// A tile starts WU = ceil(2.5 LR) columns before t0 (or at column 0) from
// H(i, .) = -2 i, as column 0 does; from t0 on its values are the untiled ones
// (ccsx_scan.h).  Consecutive jobs sit on consecutive lanes, so a
// wave may hold tiles of several reads; lanes of a short last tile idle.
//
// The text is one code per byte.  A lane reads its stretch as 8-byte words, one
// word ahead of the column it works on; per pattern pass that is one load per 8
// columns of LR cells each.  No LDS, no cross-lane traffic.
//
// A lane whose bottom row reaches the threshold at an emitted column takes a
// slot from the slice's counter (atomicAdd) and stores the record if the slot
// is inside the buffer; the counter counts them all, so the host knows the
// capacity a second run needs.  TRACK: the bottom row of every pattern and
// column goes out as int8 as well (tests and tools/scan_bench.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ccsx_scan.h"

namespace ccsx_scan {

// One pattern over one tile: the columns s + 1 .. jend of the lane's read, of
// which those from t0 on are emitted.  tp = the text from column s + 1's base
// (text[s]) on, 8-byte aligned.  MIXED: the pattern is shorter than LR.
template <int LR, bool MIXED, bool TRACK>
__device__ __forceinline__ void tile_dp(const Pat &t, uint32_t p, const uint2 *tp, int s, int t0, int jend, uint32_t read,
                                        int8_t *trk, const Args &a)
{
    const int skip = LR - t.len;  // rows 1 .. skip are row 0 again
    int h[LR];                    // h[i - 1] = H(i, j)
#pragma unroll
    for (int i = 1; i <= LR; ++i) h[i - 1] = MIXED ? (i > skip ? -kPenalty * (i - skip) : 0) : -kPenalty * i;
    if (TRACK && t0 == 0) trk[0] = (int8_t)h[LR - 1];
    uint2 nx = tp[0];
    uint64_t w = 0;
#pragma unroll 1
    for (int j = s + 1, k = 0; j <= jend; ++j, ++k) {
        if ((k & 7) == 0) {
            w = (uint64_t)nx.y << 32 | nx.x;
            nx = tp[(k >> 3) + 1];  // (inside text_bytes(n))
        }
        const uint32_t yc = (uint32_t)w;
        w >>= 8;
        // bit r of m: row r + 1's base equals the column's
        const uint64_t n0 = (yc & 1u) ? 0ull : ~0ull, n1 = (yc & 2u) ? 0ull : ~0ull;
        const uint64_t m = (t.p0 ^ n0) & (t.p1 ^ n1) & t.act;
        int diag = 0, up = 0;  // H(0, j - 1), H(0, j)
#pragma unroll
        for (int i = 1; i <= LR; ++i) {
            const int left = h[i - 1];
            const int bit = (int)((m >> (i - 1)) & 1u);
            // max(diag + s, up - 2, left - 2) with s = 3 bit - 2
            int v = max(max(diag + (kMatch + kPenalty) * bit, up), left);
            v -= MIXED ? (i > skip ? kPenalty : 0) : kPenalty;
            diag = left, up = v, h[i - 1] = v;
        }
        if (j >= t0) {
            if (TRACK) trk[j] = (int8_t)up;
            if (up >= t.thr) {
                const unsigned long long slot = atomicAdd(a.count, 1ull);
                if (slot < a.cap) a.cand[slot] = Cand{read << kPatBits | p, (uint32_t)up << kColBits | (uint32_t)j};
            }
        }
    }
}

template <int LR, bool TRACK>
__global__ __launch_bounds__(64) void scan(const Args a)
{
    constexpr int WU = (int)warmup_of(LR);
    const uint32_t g = blockIdx.x * kLanes + threadIdx.x;
    if (g >= a.njobs) return;
    const Job jb = a.jobs[g];
    const int n = (int)a.rlen[jb.read];
    const int t0 = (int)jb.t0;
    const int s = max(0, t0 - WU);
    const int jend = min(t0 + (int)kTC - 1, n);
    const uint2 *tp = reinterpret_cast<const uint2 *>(a.text + (uint64_t)a.roff[jb.read] * 8u + (uint32_t)s);
    for (uint32_t p = 0; p < a.npat; ++p) {
        const Pat t = a.pats[p];
        int8_t *trk = TRACK ? a.track + a.toff[jb.read] + (uint64_t)p * (uint32_t)(n + 1) : nullptr;
        if (t.len != LR) tile_dp<LR, true, TRACK>(t, p, tp, s, t0, jend, jb.read, trk, a);
        else tile_dp<LR, false, TRACK>(t, p, tp, s, t0, jend, jb.read, trk, a);
    }
}

template <int LR>
static void launch(const Args &a, bool track, uint32_t blocks, hipStream_t s)
{
    if (track) hipLaunchKernelGGL((scan<LR, true>), dim3(blocks), dim3(kLanes), 0, s, a);
    else hipLaunchKernelGGL((scan<LR, false>), dim3(blocks), dim3(kLanes), 0, s, a);
}

}  // namespace ccsx_scan

// rows = ccsx_scan::rows_of(the set's longest adapter): 16, 32, 48 or 64
extern "C" hipError_t ccsx_launch_scan(const ccsx_scan::Args *a, uint32_t rows, int track, hipStream_t s)
{
    if (!a->njobs) return hipSuccess;
    const uint32_t blocks = (a->njobs + ccsx_scan::kLanes - 1) / ccsx_scan::kLanes;
    switch (rows) {
    case 16: ccsx_scan::launch<16>(*a, track != 0, blocks, s); break;
    case 32: ccsx_scan::launch<32>(*a, track != 0, blocks, s); break;
    case 48: ccsx_scan::launch<48>(*a, track != 0, blocks, s); break;
    case 64: ccsx_scan::launch<64>(*a, track != 0, blocks, s); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
