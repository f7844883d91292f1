// ccsx_ref.hip -- MI355X (gfx950) vote kernel of the reference mapper.
//
// SPEC.md §18's seed for many reads per launch: one 256-thread workgroup per
// read (a grid-stride loop over the slice's reads) covers both orientations.
// Threads are strided over the read's 13-mer windows.  A window's forward
// k-mer and, from the same 13 bases, the k-mer of the reverse complement's
// window n - 13 - p are looked up in the set's sorted table: the directory on
// a k-mer's top 16 bits gives the table range, a binary search inside it the
// first equal entry.  Every equal entry (g, pos) votes for the key
// (2 g + o) << 23 | (bin + 2^22), bin = floor((pos - qpos) / 32) by an
// arithmetic shift.
//
// Votes are counted in an LDS hash table of `slots` keys (open addressing,
// linear probing): atomicCAS claims a slot for a key, atomicAdd counts.  The
// set of (key, count) pairs in the table does not depend on the order of the
// atomics; where a key lies does, and nothing reads that.  An insertion fails
// only if every slot holds another key, that is iff the read has more than
// `slots` distinct keys: the read is then flagged and the host maps it.
//
// The winner is a keyed reduction: the largest count << 32 | ~key over the
// table (the most votes, then the smallest 2 g + o, then the smallest bin,
// which is the per-pair rule and the rule over pairs at once); votes2 is the
// largest count over keys of another target.  The workgroup also writes the
// reverse complement of the read, and its last step finishes the read's band
// job (ccsx_align.hip): query = the read in the winning orientation, target,
// d0; a read without a vote, or a flagged one, gets a job of length 0.
//
// Bounds: table and directory indices are clamped to the uploaded sizes (nent,
// kDirSize); g is checked against ntarget; window loads stay inside [0, n).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ccsx_ref.h"

namespace ccsx_ref {

__device__ __forceinline__ uint32_t slot_of(uint32_t key, uint32_t mask) { return (key * 2654435761u >> 12) & mask; }

// one vote for key; false if the table holds `mask + 1` other keys
__device__ __forceinline__ bool cast(uint32_t *keys, uint32_t *cnt, uint32_t mask, uint32_t key)
{
    uint32_t s = slot_of(key, mask);
    for (uint32_t probe = 0; probe <= mask; ++probe) {
        const uint32_t old = atomicCAS(&keys[s], kEmpty, key);
        if (old == kEmpty || old == key) {
            atomicAdd(&cnt[s], 1u);
            return true;
        }
        s = (s + 1u) & mask;
    }
    return false;
}

// the votes of k-mer h at query position qp of orientation o
__device__ __forceinline__ bool lookup(const Args &a, uint32_t *keys, uint32_t *cnt, uint32_t mask, uint32_t h, int32_t qp, uint32_t o)
{
    const uint32_t b = h >> kDirShift;  // < kDirSize - 1: h has 26 bits
    uint32_t lo = min(a.dir[b], a.nent), hi = min(a.dir[b + 1], a.nent);
    const uint32_t end = hi;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.kmer[mid] < h) lo = mid + 1;
        else hi = mid;
    }
    for (; lo < end && a.kmer[lo] == h; ++lo) {
        const uint32_t e = a.gpos[lo], g = e >> kPosBits;
        if (g >= a.ntarget) continue;
        const int32_t d = (int32_t)(e & ((1u << kPosBits) - 1u)) - qp;
        if (!cast(keys, cnt, mask, (2u * g + o) << kPairShift | (uint32_t)((d >> kBinShift) + (int32_t)kBinBias))) return false;
    }
    return true;
}

__global__ __launch_bounds__(kVoteThreads) void vote(const Args a)
{
    // one array: the keys, the counts, then the two reductions and the flag
    __shared__ unsigned long long lds[kVoteSlots + 3];
    uint32_t *keys = reinterpret_cast<uint32_t *>(lds), *cnt = keys + kVoteSlots;
    unsigned long long *top = lds + kVoteSlots;  // [0] the winner, [1] votes2, [2] overflow
    const uint32_t tid = threadIdx.x;
    const uint32_t slots = min(max(a.slots, kMinVoteSlots), kVoteSlots), mask = slots - 1u;
    for (uint32_t r = blockIdx.x; r < a.nreads; r += gridDim.x) {
        const Read rd = a.reads[r];
        const int32_t n = (int32_t)rd.n;
        const uint8_t *q = a.seq + rd.fwd;
        uint8_t *rc = a.seq + rd.rc;
        for (uint32_t s = tid; s < slots; s += kVoteThreads) keys[s] = kEmpty, cnt[s] = 0;
        if (tid < 3) top[tid] = 0;
        __syncthreads();
        // the reverse complement (a code above 3 stays what it is)
        for (int32_t i = (int32_t)tid; i < n; i += (int32_t)kVoteThreads) {
            const uint32_t c = q[n - 1 - i];
            rc[i] = (uint8_t)(c < 4u ? 3u - c : c);
        }
        bool ok = true;
        for (int32_t p = (int32_t)tid; ok && p + kK <= n; p += (int32_t)kVoteThreads) {
            uint32_t hf = 0, hr = 0;
            bool valid = true;
#pragma unroll
            for (int k = 0; k < kK; ++k) {
                const uint32_t c = q[p + k];
                valid = valid && c < 4u;
                hf = hf << 2 | (c & 3u);
                hr |= (3u - (c & 3u)) << (2 * k);
            }
            if (!valid) continue;
            ok = lookup(a, keys, cnt, mask, hf, p, 0u) && lookup(a, keys, cnt, mask, hr, n - kK - p, 1u);
        }
        if (!ok) atomicMax(&top[2], 1ull);
        __syncthreads();
        // the winner: most votes, then the smallest key
        unsigned long long mine = 0;
        for (uint32_t s = tid; s < slots; s += kVoteThreads)
            if (keys[s] != kEmpty) mine = max(mine, (unsigned long long)cnt[s] << 32 | (uint32_t)~keys[s]);
        if (mine) atomicMax(&top[0], mine);
        __syncthreads();
        const unsigned long long win = top[0];
        const uint32_t wkey = ~(uint32_t)win, wg = wkey >> (kPairShift + 1);
        unsigned long long other = 0;
        for (uint32_t s = tid; s < slots; s += kVoteThreads)
            if (keys[s] != kEmpty && (keys[s] >> (kPairShift + 1)) != wg) other = max(other, (unsigned long long)cnt[s]);
        if (win && other) atomicMax(&top[1], other);
        __syncthreads();
        if (tid == 0) {
            const bool overflow = top[2] != 0, mapped = win != 0 && !overflow;
            Vote v;
            v.g = -1, v.o = 0, v.d0 = 0, v.votes = 0, v.votes2 = 0, v.overflow = overflow, v.pad[0] = v.pad[1] = 0;
            ccsx_aln::Job jb = a.jobs[r];  // rec_off and the words' offset are the host's
            jb.q_off = rd.fwd, jb.t_off = 0, jb.qlen = 0, jb.tlen = 0, jb.d0 = 0;
            if (mapped && wg < a.ntarget) {
                v.g = (int32_t)wg, v.o = (int32_t)((wkey >> kPairShift) & 1u);
                v.d0 = ((int32_t)(wkey & ((1u << kPairShift) - 1u)) - (int32_t)kBinBias) * 32 + 16;
                v.votes = (int32_t)(win >> 32), v.votes2 = (int32_t)top[1];
                jb.q_off = v.o ? rd.rc : rd.fwd, jb.t_off = a.toff[wg];
                jb.qlen = rd.n, jb.tlen = a.tlen[wg], jb.d0 = v.d0;
            }
            a.votes[r] = v;
            a.jobs[r] = jb;
        }
        __syncthreads();  // the next read clears the table
    }
}

}  // namespace ccsx_ref

extern "C" hipError_t ccsx_launch_ref_vote(const ccsx_ref::Args *a, uint32_t blocks, hipStream_t s)
{
    hipLaunchKernelGGL(ccsx_ref::vote, dim3(blocks), dim3(ccsx_ref::kVoteThreads), 0, s, *a);
    return hipGetLastError();
}
