// ccsx_barcode.hip -- MI355X (gfx950) kernel of the demultiplexer (SPEC.md
// §16): every pattern of the barcode set (each barcode and its reverse
// complement) against one end window of a CCS read, the best pattern, its
// score and end column, and the best pattern of another barcode.
// host/barcode.cpp is the same definition as a sequential loop; both give the
// same five values per (ZMW, end).
//
// One 64-lane wave per job (ZMW, end), a grid-stride loop over the slice's
// jobs; the wave walks the set in chunks of 64 patterns, one pattern per lane.
// A lane keeps its pattern as two bit planes (bit 0 / bit 1 of each base's
// code, one bit per row) and the column H(1 .. LR, j) of its DP in LR VGPRs
// (LR = the set's longest barcode rounded up to 16: the kernel is compiled for
// 16, 32, 48 and 64 rows).  The window's bases are loaded 64 at a time, one
// per lane, and the column's base is read back by v_readlane: it is the same
// for every lane, so the match bits of all rows are three bitwise operations
// per plane, and a cell is its match bit, one multiply-add, a max3 and the
// penalty.  No LDS and no cross-lane traffic inside a column.
//
// Patterns shorter than LR are right-aligned (ccsx_barcode.h): the rows above
// a pattern's first stay 0, as the definition's row 0 does, so the score of
// every lane is in row LR.  A chunk whose patterns all have LR bases runs the
// body without the per-row test (wave-uniform branch).
//
// A lane tracks the largest H(L, j) and the first column that reached it.  Per
// chunk, two wave reductions over the lanes' keys (ccsx_barcode.h: score, then
// the smallest p): the largest, and the largest among the lanes of another
// barcode.  A barcode's two patterns are adjacent lanes of one chunk, so the
// running pair (best, best of another barcode) merges chunk by chunk: a chunk
// whose best is larger takes over and the old best becomes a candidate for
// second, else the chunk's best is one.  Chunks come in increasing p and only
// a strictly larger key takes over, so equal scores keep the smallest p.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ccsx_barcode.h"

namespace ccsx_bc {

// ----------------------------------------------------------------------------
// wave primitives (gfx9 DPP), restated from ccsx_align.hip
// ----------------------------------------------------------------------------
template <int CTRL, int RM = 0xF>
__device__ __forceinline__ int dpp_max(int v)
{
    return max(v, __builtin_amdgcn_update_dpp(INT32_MIN, v, CTRL, RM, 0xF, false));
}

__device__ __forceinline__ int wave_max(int v)
{
    v = dpp_max<0x111>(v);
    v = dpp_max<0x112>(v);
    v = dpp_max<0x114>(v);
    v = dpp_max<0x118>(v);
    v = dpp_max<0x142, 0xA>(v);
    v = dpp_max<0x143, 0xC>(v);
    return __builtin_amdgcn_readlane(v, 63);
}

__device__ __forceinline__ int rdlane(int v, int l) { return __builtin_amdgcn_readlane(v, l); }

// One chunk against one window: the lane's pattern t (right-aligned in LR
// rows) against y[0 .. w).  best = max_j H(L, j), bestj = the smallest such j.
// MIXED: some lane's pattern is shorter than LR.
template <int LR, bool MIXED>
__device__ __forceinline__ void chunk_dp(const Pat &t, const uint8_t *y, int w, int lane, int &best, int &bestj)
{
    const int skip = LR - t.len;  // rows 1 .. skip are row 0 again
    int h[LR];                    // h[i - 1] = H(i, j)
#pragma unroll
    for (int i = 1; i <= LR; ++i) h[i - 1] = MIXED ? (i > skip ? -kPenalty * (i - skip) : 0) : -kPenalty * i;
    best = h[LR - 1], bestj = 0;
    for (int j0 = 0; j0 < w; j0 += (int)kLanes) {
        // (j0 + lane < w <= wn: inside the job's window)
        const int yv = j0 + lane < w ? (int)y[j0 + lane] : 0;
        const int nc = min((int)kLanes, w - j0);
#pragma unroll 1
        for (int jj = 0; jj < nc; ++jj) {
            const int yc = rdlane(yv, jj);
            // bit r of m: row r + 1's base equals the column's
            const uint64_t n0 = (yc & 1) ? 0ull : ~0ull, n1 = (yc & 2) ? 0ull : ~0ull;
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
            if (up > best) best = up, bestj = j0 + jj + 1;
        }
    }
}

template <int LR>
__global__ __launch_bounds__(64) void score(const Args a)
{
    const int lane = (int)threadIdx.x;
    for (uint32_t job = blockIdx.x; job < a.njobs; job += gridDim.x) {
        const int w = __builtin_amdgcn_readfirstlane((int)a.wlen[job >> 1]);
        const uint8_t *y = a.win + (uint64_t)job * a.wn;
        int k1 = 0, k2 = 0, e1 = 0;  // the best key so far, the best of another barcode, the best's end
        for (uint32_t c = 0; c < a.nchunks; ++c) {
            const int p = (int)(c * kLanes) + lane;
            const Pat t = a.pats[p];
            int best, bestj;
            if (__any(t.len != 0 && t.len != LR)) chunk_dp<LR, true>(t, y, w, lane, best, bestj);
            else chunk_dp<LR, false>(t, y, w, lane, best, bestj);
            const int key = t.len ? (best + kBias) << kKeyBits | (kKeyMask - p) : 0;
            const int c1 = wave_max(key);
            const int p1 = kKeyMask - (c1 & kKeyMask);
            const int c2 = wave_max((p >> 1) == (p1 >> 1) ? 0 : key);
            const int ce = rdlane(bestj, p1 & (int)(kLanes - 1));
            if (c1 > k1) {
                k2 = max(k1, c2);
                k1 = c1, e1 = ce;
            } else {
                k2 = max(k2, c1);
            }
        }
        // five words per job, one per lane
        int v = kKeyMask - (k1 & kKeyMask);
        if (lane == 1) v = (k1 >> kKeyBits) - kBias;
        if (lane == 2) v = e1;
        if (lane == 3) v = k2 ? (k2 >> kKeyBits) - kBias : kNone;
        if (lane == 4) v = k2 ? kKeyMask - (k2 & kKeyMask) : -1;
        if (lane < 5) a.out[(uint64_t)job * 5 + (uint32_t)lane] = v;
    }
}

}  // namespace ccsx_bc

// rows = ccsx_bc::rows_of(the set's longest barcode): 16, 32, 48 or 64
extern "C" hipError_t ccsx_launch_barcode(const ccsx_bc::Args *a, uint32_t rows, uint32_t blocks, hipStream_t s)
{
    switch (rows) {
    case 16: hipLaunchKernelGGL(ccsx_bc::score<16>, dim3(blocks), dim3(64), 0, s, *a); break;
    case 32: hipLaunchKernelGGL(ccsx_bc::score<32>, dim3(blocks), dim3(64), 0, s, *a); break;
    case 48: hipLaunchKernelGGL(ccsx_bc::score<48>, dim3(blocks), dim3(64), 0, s, *a); break;
    case 64: hipLaunchKernelGGL(ccsx_bc::score<64>, dim3(blocks), dim3(64), 0, s, *a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
