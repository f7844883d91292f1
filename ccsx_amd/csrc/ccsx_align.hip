// ccsx_align.hip -- MI355X (gfx950) band aligner for ccs_prepare's strand check.
//
// SPEC.md §8 steps 2-3 (ccsx_pairwise_band, host/pairwise.cpp) for many pairs
// per launch: one 64-lane wave per job, a grid-stride loop over the slice's
// jobs.  The 513 band cells of a query row lie on lanes 0..56, nine adjacent
// cells per lane (cell k on lane k / 9); lanes 57..63 hold cells outside the
// band, which stay 0.
//
// A row: every lane forms E = max(0, diag, up) of its cells from the previous
// row's H in registers (up of its last cell from the next lane's first, one
// DPP shift).  The in-row chain H(k) = max(E(k), H(k-1) - 2) is
// max_{k' <= k} E(k') - 2 (k - k'): per lane the value its run hands on, an
// exclusive DPP max-scan of that plus 18 x lane over the wave, then one pass
// along the lane's cells.  The direction is E's unless left is strictly
// larger, as in the sequential loop (ties: diag, up, left).  The target
// window is nine 3-bit codes in one register per lane and slides one base per
// row: a lane's new last code is the next lane's first; lane 56 takes the base
// entering the band, loaded 64 rows ahead with the query (one base per lane,
// read back by v_readlane).  Codes: 0..3 a base, 4 a target base that never
// matches, 5 no target base there (j outside [0, tlen): H = 0, dir = 0); a
// query code >= 4 becomes 7.  Every load of q and t is guarded by i < qlen and
// 0 <= j < tlen.
//
// Each lane keeps the first strict maximum over its cells in row order; at the
// end the wave takes the largest score, then the smallest row, then the
// smallest cell: the first cell in row-major order that exceeds every earlier
// one.  Each row's directions go to the job's records in the arena: one word
// per lane and row (nine 3-bit records), 256 bytes per row.  The traceback
// (pairwise.cpp's loop, step for step) copies 32 record rows at a time into
// LDS and walks them with all lanes in step.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "ccsx_align.h"

namespace ccsx_aln {

// ----------------------------------------------------------------------------
// wave primitives (gfx9 DPP), restated from ccsx_kernel.hip
// ----------------------------------------------------------------------------
template <int CTRL, int RM = 0xF>
__device__ __forceinline__ int dpp_max(int v)
{
    return max(v, __builtin_amdgcn_update_dpp(INT32_MIN, v, CTRL, RM, 0xF, false));
}

// inclusive max-scan over the 64 lanes
__device__ __forceinline__ int wave_incl_max(int v)
{
    v = dpp_max<0x111>(v);
    v = dpp_max<0x112>(v);
    v = dpp_max<0x114>(v);
    v = dpp_max<0x118>(v);
    v = dpp_max<0x142, 0xA>(v);
    return dpp_max<0x143, 0xC>(v);
}

// lane l <- l-1 (lane 0 <- old); lane l <- l+1 (lane 63 <- old)
__device__ __forceinline__ int wave_shr1(int old, int v) { return __builtin_amdgcn_update_dpp(old, v, 0x138, 0xF, 0xF, false); }
__device__ __forceinline__ int wave_shl1(int old, int v) { return __builtin_amdgcn_update_dpp(old, v, 0x130, 0xF, 0xF, false); }

__device__ __forceinline__ int wave_max(int v) { return __builtin_amdgcn_readlane(wave_incl_max(v), 63); }
__device__ __forceinline__ int wave_min(int v) { return -wave_max(-v); }

constexpr int kNeg = -(1 << 29);  // below every score, far from overflow
constexpr uint32_t kMapMismatch = 0x40000000u, kMapIns = 0x80000000u;  // CCSX_MAP_MISMATCH, CCSX_MAP_INS
constexpr int kC = kCellsPerLane;

__device__ __forceinline__ uint32_t tcode(const uint8_t *t, int tlen, int j, bool lane_in_band)
{
    if (!lane_in_band || j < 0 || j >= tlen) return 5u;
    const uint32_t b = t[j];
    return b < 4u ? b : 4u;
}

// PATH: the traceback also stores the §11 word of every query base it consumes
// and the wave then fills the clipped ends (SPEC.md §18); PATH = false is the
// aligner's kernel, instruction for instruction (it keeps Args: a longer
// argument block would move the hidden arguments behind it)
template <bool PATH>
__global__ __launch_bounds__(64) void band_align(const std::conditional_t<PATH, PathArgs, Args> a)
{
    uint32_t *words = nullptr;
    if constexpr (PATH) words = a.words;
    __shared__ uint32_t tbuf[kTbRows * kRowWords];
    const int lane = (int)threadIdx.x;
    const bool in_band = lane < kBandLanes;
    for (uint32_t job = blockIdx.x; job < a.njobs; job += gridDim.x) {
        const Job jb = a.jobs[job];
        const uint8_t *q = a.seq + jb.q_off, *t = a.seq + jb.t_off;
        uint32_t *rec = a.rec + jb.rec_off;
        const int qlen = (int)jb.qlen, tlen = (int)jb.tlen;
        const int lo = jb.d0 - kHalfBand;
        // the target window of row 0: cell c of this lane is k = 9 lane + c, j = lo + k
        uint32_t tw = 0;
#pragma unroll
        for (int c = 0; c < kC; ++c) tw |= tcode(t, tlen, lo + kC * lane + c, in_band) << (3 * c);
        int H[kC];
#pragma unroll
        for (int c = 0; c < kC; ++c) H[c] = 0;
        int best = 0, bpos = 0;  // bpos = row << 4 | cell of the lane
        for (int i0 = 0; i0 < qlen; i0 += 64) {
            // this block's query bases and the target bases entering the band
            // at k = 512 after each of its rows, one per lane
            const int qi = i0 + lane;
            uint32_t qv = 7u;
            if (qi < qlen) {
                const uint32_t b = q[qi];
                qv = b < 4u ? b : 7u;
            }
            const uint32_t tv = tcode(t, tlen, qi + 1 + lo + (kBand - 1), true);
            const int nr = min(64, qlen - i0);
#pragma unroll 1
            for (int r = 0; r < nr; ++r) {
                const int i = i0 + r;
                const uint32_t qb = (uint32_t)__builtin_amdgcn_readlane((int)qv, r);
                const int hn = wave_shl1(0, H[0]);  // P(i-1, k+1) of the lane's last cell
                int E[kC];
                uint32_t D[kC];
                int T = kNeg;
#pragma unroll
                for (int c = 0; c < kC; ++c) {
                    const uint32_t tc = (tw >> (3 * c)) & 7u;
                    const bool m = tc == qb;
                    const int diag = H[c] + (m ? 1 : -2);
                    const int up = (c + 1 < kC ? H[c + 1] : hn) - 2;
                    int e = 0;
                    uint32_t d = 0;
                    if (diag > e) e = diag, d = m ? 5u : 1u;
                    if (up > e) e = up, d = 2u;
                    if (tc == 5u) e = 0, d = 0;
                    E[c] = e, D[c] = d;
                    T = max(T, e - 2 * (kC - 1 - c));
                }
                // what the lanes before this one hand on to its first cell: H(k-1) - 2
                const int g = wave_shr1(kNeg, wave_incl_max(T + 2 * kC * lane));
                int left = g - 2 * kC * lane + 2 * (kC - 1);
                uint32_t word = 0;
#pragma unroll
                for (int c = 0; c < kC; ++c) {
                    int v = E[c];
                    uint32_t d = D[c];
                    if (left > v) v = left, d = 3u;
                    if (((tw >> (3 * c)) & 7u) == 5u) v = 0, d = 0;
                    H[c] = v;
                    word |= d << (3 * c);
                    left = v - 2;
                    if (v > best) best = v, bpos = (i << 4) | c;
                }
                if (in_band) rec[(uint64_t)i * kRowWords + lane] = word;
                // slide the window one target base
                const uint32_t tin = (uint32_t)__builtin_amdgcn_readlane((int)tv, r);
                uint32_t inc = (uint32_t)wave_shl1(5, (int)(tw & 7u));
                if (lane == kBandLanes - 1) inc = tin;
                if (!in_band) inc = 5u;
                tw = (tw >> 3) | (inc << (3 * (kC - 1)));
            }
        }
        // the best cell: largest score, then smallest row, then smallest cell
        const int m = wave_max(best);
        int32_t res[10];
#pragma unroll
        for (int f = 0; f < 10; ++f) res[f] = 0;
        if (m > 0) {
            const bool top = best == m;
            const int bi = wave_min(top ? (bpos >> 4) : INT32_MAX);
            const int bk = wave_min(top && (bpos >> 4) == bi ? kC * lane + (bpos & 15) : INT32_MAX);
            // the wave's record stores must have landed before it reads them back
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            __syncthreads();
            int i = bi, k = bk;
            int qb = 0, tb = 0, mat = 0, mis = 0, ins = 0, del = 0;
            int blk_lo = bi + 1;  // nothing staged yet
            for (;;) {
                if (i < blk_lo) {
                    // stage rows [blk_lo, blk_lo + 32) that end at row i
                    __syncthreads();
                    blk_lo = max(0, i - (int)kTbRows + 1);
                    const int rows = i - blk_lo + 1;
                    for (int rr = 0; rr < rows; ++rr)
                        tbuf[rr * kRowWords + lane] = rec[(uint64_t)(blk_lo + rr) * kRowWords + lane];
                    __syncthreads();
                }
                const uint32_t w = tbuf[(i - blk_lo) * kRowWords + k / kC];
                const uint32_t d = (w >> (3 * (k % kC))) & 7u;
                const uint32_t dir = d & 3u;
                if (dir == 0) break;
                const int j = i + lo + k;
                if (dir == 1) {
                    if (d & 4u) ++mat;
                    else ++mis;
                    if (PATH && lane == 0) words[jb.pad + (uint32_t)i] = (uint32_t)j | (d & 4u ? 0u : kMapMismatch);
                    qb = i, tb = j;
                    --i;
                } else if (dir == 2) {
                    ++ins;
                    if (PATH && lane == 0) words[jb.pad + (uint32_t)i] = kMapIns | (uint32_t)(j + 1);
                    qb = i;
                    --i, ++k;
                } else {
                    ++del;
                    tb = j;
                    --k;
                }
                if (i < 0 || k < 0 || k >= kBand) break;
            }
            res[0] = qb, res[1] = bi + 1, res[2] = tb, res[3] = bi + lo + bk + 1;
            res[4] = mat, res[5] = mis, res[6] = ins, res[7] = del;
            res[8] = mat + mis + ins + del, res[9] = m;
        }
        if (lane == 0) {
#pragma unroll
            for (int f = 0; f < 10; ++f) a.out[(uint64_t)job * 10 + f] = res[f];
        }
        if (PATH) {
            // the clipped ends: before qb the words point at tb, from qe on at te
            // (the all-zero result: at 0 throughout)
            for (int w = lane; w < res[0]; w += 64) words[jb.pad + (uint32_t)w] = kMapIns | (uint32_t)res[2];
            for (int w = res[1] + lane; w < qlen; w += 64) words[jb.pad + (uint32_t)w] = kMapIns | (uint32_t)res[3];
        }
        __syncthreads();  // the next job's traceback reuses tbuf
    }
}

}  // namespace ccsx_aln

extern "C" hipError_t ccsx_launch_band_align(const ccsx_aln::Args *a, uint32_t blocks, hipStream_t s)
{
    hipLaunchKernelGGL(ccsx_aln::band_align<false>, dim3(blocks), dim3(64), 0, s, *a);
    return hipGetLastError();
}

// the path variant (the reference mapper, ccsx_ref.cpp): a->words receives the path
extern "C" hipError_t ccsx_launch_band_align_path(const ccsx_aln::PathArgs *a, uint32_t blocks, hipStream_t s)
{
    hipLaunchKernelGGL(ccsx_aln::band_align<true>, dim3(blocks), dim3(64), 0, s, *a);
    return hipGetLastError();
}
