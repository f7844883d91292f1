// ccsx_scan.h -- what the adapter scanner's kernel (ccsx_scan.hip), its host
// side (ccsx_scan.cpp) and the host restatement (host/scan.cpp) share: SPEC.md
// §17's constants, the pattern table, the tiling, the slice layout in the
// scanner's arena, the candidate record and the launcher.  DESIGN.md §21
// describes the layout.
#ifndef CCSX_SCAN_H
#define CCSX_SCAN_H
#include <stdint.h>

#include "ccsx_polish.h"  // ccsx_pol::base_code (SPEC.md §1's coding)

namespace ccsx_scan {

constexpr uint32_t kMaxSet = 64;     // A
constexpr uint32_t kMaxLen = 64;     // L_a
constexpr int kMatch = 1, kPenalty = 2;  // s = +1 / -2, gaps -2
constexpr int kDefT = 75, kDefLmin = 50;
constexpr uint32_t kLanes = 64;

// The tiling.  A lane emits the columns [t0, t0 + kTC) of one read and starts
// its DP at column max(0, t0 - WU), WU = ceil(2.5 LR), with H(i, .) = -2 i as
// column 0 has: an optimal alignment into (i, j) spans at most 2.5 i columns
// (SPEC.md §17), so from t0 on the tile's values are the untiled ones.  kTC and
// every WU are multiples of 8: a lane's text starts on an 8-byte word.
constexpr uint32_t kTC = 512;
inline uint32_t rows_of(uint32_t maxlen) { return (maxlen + 15u) / 16u * 16u; }
#if defined(__HIPCC__)
__host__ __device__
#endif
constexpr uint32_t warmup_of(uint32_t rows) { return (5u * rows + 1u) / 2u; }  // 40, 80, 120, 160

// A candidate in the slice's buffer: two words.  w0 = read << 7 | pattern
// (read = its index in the slice), w1 = score << 24 | column.  So a read has
// at most kMaxCol bases and a slice at most kMaxReads reads.
constexpr uint32_t kColBits = 24, kMaxCol = (1u << kColBits) - 1u;
constexpr uint32_t kPatBits = 7, kMaxReads = 1u << (32 - kPatBits);
struct Cand {
    uint32_t w0, w1;
};

// One pattern, right-aligned in LR rows as ccsx_barcode.h's is: base k of its L
// bases is row LR - L + 1 + k, bit (row - 1) of p0 / p1 holds bit 0 / 1 of that
// base's code, act has the bits of its L rows.  thr = the smallest score S with
// 100 S >= T L.
struct Pat {
    uint64_t p0, p1, act;
    int32_t len, thr;
};

inline int32_t threshold_of(uint32_t L, uint32_t T) { return (int32_t)((T * L + 99u) / 100u); }

// code k of pattern p = 2 a + o of adapter x[0 .. L)
inline uint32_t pat_code(const char *x, uint32_t L, uint32_t o, uint32_t k)
{
    return o ? 3u - ccsx_pol::base_code((uint8_t)x[L - 1 - k]) : ccsx_pol::base_code((uint8_t)x[k]);
}

inline Pat make_pat(const char *x, uint32_t L, uint32_t o, uint32_t LR, uint32_t T)
{
    Pat t{0, 0, 0, (int32_t)L, threshold_of(L, T)};
    const uint32_t skip = LR - L;
    for (uint32_t k = 0; k < L; ++k) {
        const uint32_t c = pat_code(x, L, o, k);
        t.p0 |= (uint64_t)(c & 1u) << (skip + k);
        t.p1 |= (uint64_t)(c >> 1) << (skip + k);
        t.act |= 1ull << (skip + k);
    }
    return t;
}

// a tile job: the columns [t0, t0 + kTC) of read `read` of the slice
struct Job {
    uint32_t read, t0;
};

// the text of a read of n bases takes this many bytes of the slice (codes
// 0..3, one per byte): the kernel loads 8-byte words and one word ahead
inline uint64_t text_bytes(uint32_t n) { return ((uint64_t)n + 7u) / 8u * 8u + 16u; }

struct Args {
    const Pat *pats;        // npat patterns (the set: uploaded by ccsx_gpu_scan_set)
    const uint8_t *text;    // read r at text + 8 * roff[r]
    const uint32_t *roff;   // per read, in 8-byte words
    const uint32_t *rlen;   // per read
    const Job *jobs;        // njobs
    unsigned long long *count;  // every candidate, stored or not
    Cand *cand;             // cap records
    int8_t *track;          // TRACK: S_p(j) of read r at track + toff[r] + p * (n + 1) + j
    const uint64_t *toff;   // TRACK: per read
    uint64_t cap;
    uint32_t njobs, npat;
};

}  // namespace ccsx_scan

#ifdef CCSX_SCAN_HOST_API
// host/scan.cpp's parts that ccsx_scan.cpp uses (after include/ccsx_gpu.h)
#include <vector>

namespace ccsx_scan {

struct HostCand {
    uint32_t read, p, j;
    int32_t s;
};

// every candidate (read, p, j, S_p(j)) of one read, appended to c
void candidates(const char *seqs, const uint32_t *off, const uint32_t *len, uint32_t A, uint32_t T, const char *ccs, uint32_t n,
                uint32_t read, std::vector<HostCand> &c);
// the hits of the candidates c (any order, every candidate of the reads it
// speaks of; sorted in place), appended to out by (read, end, adapter)
void finish(std::vector<HostCand> &c, const char *seqs, const uint32_t *off, const uint32_t *len, const ccsx_scan_in *reads,
            std::vector<ccsx_scan_hit> &out);

}  // namespace ccsx_scan
#endif

#endif
