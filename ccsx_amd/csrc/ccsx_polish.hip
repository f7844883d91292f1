// ccsx_polish.hip -- MI355X (gfx950) kernels of the polish step (SPEC.md §15):
// realign every pushed segment to the draft CCS, vote per draft position,
// assemble the polished read.  host/polish.cpp is the same definition as a
// sequential loop; both give the same bytes.
//
// realign: one 64-lane wave per (ZMW, segment) job, a grid-stride loop over
// the slice's jobs; lane t holds band cell t of the current row.  The anchors
// and bases of 64 rows are loaded at a time, one per lane, and read back by
// v_readlane.  A row takes the previous row's H shifted by lo_i - lo_{i-1}
// lanes (one ds_bpermute for `up`; `diag` is that shifted one lane further by
// DPP, its lane 0 from a v_readlane), the draft codes of its 64 cells from a
// two-register window over the 128 aligned draft bases around the band
// (reloaded when the band's 64-aligned base moves), and runs the in-row chain
// H(t) = max(E(t), H(t-1) - 2) as the DPP max-scan of E + 2t.  The direction
// is E's unless left is strictly larger, as in the sequential loop.  A row's
// directions are two ballots (bit 0 and bit 1 of the 64 cells); the lane whose
// row it is keeps them, and the 64 rows go out together, 16 bytes per lane.
// At a piece break and at the end, the end cell of the finished piece (largest
// H, smallest t) is stored for its last row.
//
// The traceback walks wave-uniformly from the last piece's end cell.  It
// stages 64 record rows at a time in lane registers (row blk + lane on lane
// `lane`: its two masks, its lo, its base, whether it starts a piece), reads
// the current row's by v_readlane, and collects w' and the piece's last
// aligned offset on the row's lane; a block's 64 entries get their mismatch
// bit (one draft load per lane) and go out together.  No index into memory
// depends on a record: a cell index is clamped to the band, and the draft is
// read at offsets < n only.
//
// vote: a workgroup per job; a thread per base adds its entry to the ZMW's
// counters with atomics; the thread of a piece's first row (always an aligned
// entry, §15) adds the piece's range to cov / covs as differences.
// assemble: a workgroup per ZMW; 256 positions at a time: prefix sums of the
// cov / covs differences, 0..2 output bytes per position, a prefix sum of the
// lengths, then bases, qualities and counts.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ccsx_layout.h"
#include "ccsx_polish.h"

namespace ccsx_pol {

// ----------------------------------------------------------------------------
// wave primitives (gfx9 DPP), restated from ccsx_align.hip
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

// lane l <- l-1 (lane 0 <- old)
__device__ __forceinline__ int wave_shr1(int old, int v) { return __builtin_amdgcn_update_dpp(old, v, 0x138, 0xF, 0xF, false); }

__device__ __forceinline__ int wave_max(int v) { return __builtin_amdgcn_readlane(wave_incl_max(v), 63); }

__device__ __forceinline__ int rdlane(int v, int l) { return __builtin_amdgcn_readlane(v, l); }

// lane l <- v of lane (l + d) & 63
__device__ __forceinline__ int rotl(int v, int lane, int d) { return __builtin_amdgcn_ds_bpermute(((lane + d) & 63) << 2, v); }

// the end cell of a piece: the largest H of its last row, ties to the smallest t
__device__ __forceinline__ int end_cell(int H)
{
    const int mx = wave_max(H);
    return __builtin_ctzll(__ballot(H == mx));
}

__global__ __launch_bounds__(64) void realign(const Args a)
{
    const int lane = (int)threadIdx.x;
    for (uint32_t job = blockIdx.x; job < a.njobs; job += gridDim.x) {
        const Job jb = a.jobs[job];
        const Zmw z = a.zmws[jb.zmw];
        const int n = (int)z.n, m = (int)jb.m;
        const uint8_t *c = a.ccs + z.ccs_off, *r = a.seq + jb.row_off;
        const uint32_t *w = a.map + jb.row_off;
        uint64_t *rec = a.rec + 2 * jb.row_off;
        uint8_t *pend = a.pend + jb.row_off;
        int H = 0, lo_prev = 0;
        int cbase = -1;
        int c0 = 4, c1 = 4;  // the draft codes at cbase + lane and cbase + 64 + lane (4: past the end)
        for (int i0 = 0; i0 < m; i0 += 64) {
            const int ri = i0 + lane;
            int rv = 0, lov = 0;
            if (ri < m) {
                rv = (int)base_code(r[ri]);
                lov = band_lo(w[ri] & kOffset, z.n);
            }
            uint64_t m0 = 0, m1 = 0;
            const int nr = min(64, m - i0);
#pragma unroll 1
            for (int rr = 0; rr < nr; ++rr) {
                const int i = i0 + rr;
                const int lo = rdlane(lov, rr), rc = rdlane(rv, rr);
                const int d = lo - lo_prev;
                int pu = 0, pd = 0;
                if (i == 0 || d >= kBand) {
                    // a new piece; the one before ends at the previous row
                    if (i) {
                        const int te = end_cell(H);
                        if (lane == 0) pend[i - 1] = (uint8_t)te;
                    }
                } else {
                    const int sh = rotl(H, lane, d);
                    pu = lane + d < kBand ? sh : kNeg;
                    const int edge = d >= 1 ? rdlane(H, (d - 1) & 63) : kNeg;
                    pd = wave_shr1(edge, pu);
                }
                lo_prev = lo;
                const int cb = lo & ~63;
                if (cb != cbase) {
                    cbase = cb;
                    const int j0 = cb + lane, j1 = j0 + 64;
                    c0 = j0 < n ? (int)base_code(c[j0]) : 4;
                    c1 = j1 < n ? (int)base_code(c[j1]) : 4;
                }
                const int o = lo - cb;
                const int x0 = rotl(c0, lane, o), x1 = rotl(c1, lane, o);
                const int cc = lane + o < 64 ? x0 : x1;
                const bool valid = lo + lane < n;
                int e = pd + (cc == rc ? 1 : -2);
                uint32_t dr = 1;
                const int up = pu - 2;
                if (up > e) e = up, dr = 2;
                // H(t) = max over t' <= t of E(t') - 2 (t - t')
                const int g = wave_incl_max(e + 2 * lane) - 2 * lane;
                const int left = wave_shr1(kNeg + 2, g) - 2;  // NEG at t = 0
                if (left > e) dr = 3;
                H = valid ? g : kNeg;
                if (!valid) dr = 0;
                const uint64_t b0 = __ballot(dr & 1u), b1 = __ballot(dr & 2u);
                if (lane == rr) m0 = b0, m1 = b1;
            }
            if (ri < m) rec[2 * ri] = m0, rec[2 * ri + 1] = m1;
        }
        {
            const int te = end_cell(H);
            if (lane == 0) pend[m - 1] = (uint8_t)te;
        }
        // the wave's record stores must have landed before it reads them back
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
        __syncthreads();
        uint32_t *wout = a.wout + jb.row_off, *pl = a.pl + jb.row_off;
        int i = m - 1, j = 0;
        int jt = pend[i] & 63;  // the cell to start from in row i, relative to its lo
        bool rel = true, seen = false;
        uint32_t l = 0;  // the piece's last aligned offset, once seen
        while (i >= 0) {
            const int blk = i & ~63, row = blk + lane;
            uint64_t m0 = 0, m1 = 0;
            int lov = 0, fv = 0;
            uint32_t rv = 0;
            if (row < m) {
                m0 = rec[2 * row], m1 = rec[2 * row + 1];
                lov = band_lo(w[row] & kOffset, z.n);
                rv = base_code(r[row]);
                fv = row == 0 || lov - band_lo(w[row - 1] & kOffset, z.n) >= kBand;
            }
            uint32_t wv = 0, plv = 0;
            while (i >= blk) {
                const int rr = i - blk;
                const int lo = rdlane(lov, rr);
                if (rel) j = lo + jt, rel = false;
                const int t = min(max(j - lo, 0), kBand - 1);
                const uint32_t q0 = (uint32_t)rdlane((int)(uint32_t)(t < 32 ? m0 : m0 >> 32), rr);
                const uint32_t q1 = (uint32_t)rdlane((int)(uint32_t)(t < 32 ? m1 : m1 >> 32), rr);
                const uint32_t dr = ((q0 >> (t & 31)) & 1u) | (((q1 >> (t & 31)) & 1u) << 1);
                if (dr == 3u && t > 0) {
                    --j;
                    continue;
                }
                const bool first = rdlane(fv, rr) != 0;
                uint32_t ent;
                if (dr == 2u && !first) {
                    ent = kIns | ((uint32_t)(j + 1) & kOffset);
                } else {
                    ent = (uint32_t)j & kOffset;
                    if (!seen) seen = true, l = ent;
                    --j;
                }
                if (lane == rr) wv = ent, plv = seen ? l : 0u;
                if (first) {
                    seen = false;
                    if (i > 0) jt = pend[i - 1] & 63, rel = true;
                }
                --i;
            }
            if (row < m) {
                const uint32_t off = wv & kOffset;
                if (!(wv & kIns) && off < z.n && base_code(c[off]) != rv) wv |= kMismatch;
                wout[row] = wv, pl[row] = plv;
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void vote(const Args a)
{
    for (uint32_t job = blockIdx.x; job < a.njobs; job += gridDim.x) {
        const Job jb = a.jobs[job];
        const Zmw z = a.zmws[jb.zmw];
        const uint32_t n = z.n;
        const uint8_t *r = a.seq + jb.row_off;
        const uint32_t *w = a.map + jb.row_off, *wout = a.wout + jb.row_off, *pl = a.pl + jb.row_off;
        uint32_t *cnt = a.cnt + z.cnt_off;
        for (uint32_t row = threadIdx.x; row < jb.m; row += blockDim.x) {
            const uint32_t wv = wout[row], off = wv & kOffset, x = base_code(r[row]), l = pl[row];
            if (!(wv & kIns)) {
                if (off >= n) continue;
                atomicAdd(&cnt[(uint64_t)off * kCounters + kCnt + x], 1u);
                const bool first = row == 0 || band_lo(w[row] & kOffset, n) - band_lo(w[row - 1] & kOffset, n) >= kBand;
                if (first && l >= off && l < n) {
                    // cov over [off, l], covs over (off, l], as differences; l + 1 <= n
                    atomicAdd(&cnt[(uint64_t)off * kCounters + kCov], 1u);
                    atomicSub(&cnt[(uint64_t)(l + 1) * kCounters + kCov], 1u);
                    atomicAdd(&cnt[(uint64_t)(off + 1) * kCounters + kCovs], 1u);
                    atomicSub(&cnt[(uint64_t)(l + 1) * kCounters + kCovs], 1u);
                }
            } else {
                // an insertion entry follows an aligned one of its piece (a piece's
                // first row is aligned), so f < off; it counts if it is the first at
                // its slot and the slot is not past the piece's last aligned offset
                if (row == 0 || off > n || off > l) continue;
                const uint32_t pv = wout[row - 1];
                if ((pv & kIns) && (pv & kOffset) == off) continue;
                atomicAdd(&cnt[(uint64_t)off * kCounters + kInsn], 1u);
                atomicAdd(&cnt[(uint64_t)off * kCounters + kInsb + x], 1u);
            }
        }
    }
}

// inclusive sum over the workgroup's 256 threads; total = the sum of all
__device__ __forceinline__ int block_incl_sum(int v, int *sh, int &total)
{
    const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    __syncthreads();  // the last call's readers are done with sh
    if (lane == 63) sh[wv] = v;
    __syncthreads();
    int add = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < (int)kAsmThreads / 64; ++k) {
        if (k < wv) add += sh[k];
        total += sh[k];
    }
    return v + add;
}

__device__ __forceinline__ uint32_t argmax4(const uint32_t *v)
{
    uint32_t b = 0;
#pragma unroll
    for (uint32_t x = 1; x < 4; ++x)
        if (v[x] > v[b]) b = x;
    return b;
}

__global__ __launch_bounds__(kAsmThreads) void assemble(const Args a)
{
    __shared__ int sh[kAsmThreads / 64];
    for (uint32_t zi = blockIdx.x; zi < a.nzmw; zi += gridDim.x) {
        const Zmw z = a.zmws[zi];
        const uint32_t n = z.n;
        const uint8_t *c = a.ccs + z.ccs_off;
        const uint32_t *cnt = a.cnt + z.cnt_off;
        uint8_t *oseq = a.oseq + z.out_off, *oqual = a.oqual + z.out_off;
        int ccov = 0, ccovs = 0, cout = 0;  // carried over the blocks of positions
        uint32_t nsub = 0, nins = 0, ndel = 0;
        for (uint32_t g0 = 0; g0 <= n; g0 += kAsmThreads) {
            const uint32_t g = g0 + threadIdx.x;
            const bool in = g <= n;
            uint32_t v[kCounters];
#pragma unroll
            for (uint32_t k = 0; k < kCounters; ++k) v[k] = in ? cnt[(uint64_t)g * kCounters + k] : 0u;
            int tcov, tcovs, tlen;
            const uint32_t cov = (uint32_t)(ccov + block_incl_sum((int)v[kCov], sh, tcov));
            const uint32_t covs = (uint32_t)(ccovs + block_incl_sum((int)v[kCovs], sh, tcovs));
            ccov += tcov, ccovs += tcovs;
            uint8_t b[2], q[2];
            int len = 0;
            if (in) {
                if (2u * v[kInsn] > covs) {
                    const uint32_t x = argmax4(v + kInsb);
                    b[len] = (uint8_t) "ACGT"[x], q[len] = ccsx::qual_phred(v[kInsb + x], covs);
                    ++len, ++nins;
                }
                if (g < n) {
                    const uint32_t cg = base_code(c[g]);
                    if (cov == 0) {
                        b[len] = (uint8_t) "ACGT"[cg], q[len] = (uint8_t)ccsx::kQMin;
                        ++len;
                    } else {
                        const uint32_t best = argmax4(v + kCnt);
                        const uint32_t gap = cov - (v[0] + v[1] + v[2] + v[3]);
                        if (v[kCnt + best] >= gap) {
                            b[len] = (uint8_t) "ACGT"[best], q[len] = ccsx::qual_phred(v[kCnt + best], cov);
                            ++len, nsub += best != cg;
                        } else {
                            ++ndel;
                        }
                    }
                }
            }
            const int pos = cout + block_incl_sum(len, sh, tlen) - len;
            cout += tlen;
            // pos + len <= 2 g + 1 <= 2 n + 1, the ZMW's output bytes
            for (int k = 0; k < len; ++k) oseq[pos + k] = b[k], oqual[pos + k] = q[k];
        }
        uint32_t *hdr = a.hdr + 4 * (uint64_t)zi;
        if (threadIdx.x == 0) hdr[0] = (uint32_t)cout;
        if (nsub) atomicAdd(&hdr[1], nsub);
        if (nins) atomicAdd(&hdr[2], nins);
        if (ndel) atomicAdd(&hdr[3], ndel);
        __syncthreads();
    }
}

}  // namespace ccsx_pol

extern "C" hipError_t ccsx_launch_polish(const ccsx_pol::Args *a, uint32_t job_blocks, uint32_t zmw_blocks, hipStream_t s)
{
    hipLaunchKernelGGL(ccsx_pol::realign, dim3(job_blocks), dim3(64), 0, s, *a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ccsx_pol::vote, dim3(job_blocks), dim3(256), 0, s, *a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(ccsx_pol::assemble, dim3(zmw_blocks), dim3(ccsx_pol::kAsmThreads), 0, s, *a);
    return hipGetLastError();
}
