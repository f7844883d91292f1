// ccsx_polish.h -- what the polisher's kernels (ccsx_polish.hip), its host side
// (ccsx_polish.cpp) and the host restatement (host/polish.cpp) share: SPEC.md
// §15's constants, the slice layout in the polisher's arena and the launchers.
// DESIGN.md §19 describes the layout.
#ifndef CCSX_POLISH_H
#define CCSX_POLISH_H
#include <stdint.h>

namespace ccsx_pol {

constexpr int kBand = 64;            // W: one band cell per lane
constexpr int kHalf = 32;            // lo = clamp(anchor - 32, 0, max(n - 64, 0))
constexpr int kNeg = -(1 << 29);     // NEG: an invalid or out-of-band cell
constexpr uint32_t kOffset = 0x3FFFFFFFu, kMismatch = 0x40000000u, kIns = 0x80000000u;  // §11's word
// segment lengths and n below this keep the 32-bit scores far from NEG
constexpr uint32_t kMaxLen = 1u << 27;
// counters per CCS position g in [0, n]: cnt x4, cov, covs, insn, insb x4.
// cov and covs are kept as differences (+1 at a range's start, -1 past its
// end) and summed by the assemble kernel
constexpr uint32_t kCounters = 11;
constexpr uint32_t kCnt = 0, kCov = 4, kCovs = 5, kInsn = 6, kInsb = 7;
constexpr uint32_t kAsmThreads = 256;

// SPEC.md §1's coding
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t base_code(uint8_t ch)
{
    switch (ch | 0x20) {
    case 'c': return 1;
    case 'g': return 2;
    case 't':
    case 'u': return 3;
    default: return 0;
    }
}

#if defined(__HIPCC__)
__host__ __device__
#endif
inline int32_t band_lo(uint32_t anchor, uint32_t n)
{
    const int32_t hi = (int32_t)n > kBand ? (int32_t)n - kBand : 0;
    const int32_t lo = (int32_t)anchor - kHalf;
    return lo < 0 ? 0 : lo > hi ? hi : lo;
}

// a ZMW of a slice
struct Zmw {
    uint64_t ccs_off;   // bytes from Args::ccs
    uint64_t cnt_off;   // words from Args::cnt: (n + 1) * kCounters
    uint64_t out_off;   // bytes from Args::oseq / Args::oqual: 2 n + 1
    uint32_t n;
    uint32_t pad;
};

// a (ZMW, segment) job of a slice; its rows are [row_off, row_off + m)
struct Job {
    uint64_t row_off;   // rows from the start of every per-row array
    uint32_t m;
    uint32_t zmw;       // index into Args::zmws
};

struct Args {
    const Zmw *zmws;
    const Job *jobs;
    const uint8_t *ccs;    // the drafts, ASCII
    const uint8_t *seq;    // one byte per row, ASCII
    const uint32_t *map;   // one §11 word per row (the anchors)
    uint64_t *rec;         // two lane masks per row: bit t of word 0 / 1 = bit 0 / 1 of cell t's direction
    uint8_t *pend;         // the end cell of the piece whose last row this is
    uint32_t *wout;        // the realigned map
    uint32_t *pl;          // the last aligned offset of the row's piece (0 on a piece's trailing insertions)
    uint32_t *cnt;         // the counters, zeroed before the vote
    uint32_t *hdr;         // per ZMW: len, nsub, nins, ndel (zeroed)
    uint8_t *oseq, *oqual;
    uint32_t nzmw, njobs;
};

// SPEC.md §15's anchor conditions on one ZMW's map (segments back to back)
inline bool map_ok(const uint32_t *map, const uint32_t *seg_len, uint32_t nseg, uint32_t n)
{
    uint64_t o = 0;
    for (uint32_t k = 0; k < nseg; o += seg_len[k], ++k) {
        uint32_t prev = 0;
        for (uint32_t i = 0; i < seg_len[k]; ++i) {
            const uint32_t a = map[o + i] & kOffset;
            if (a < prev || a > n) return false;
            prev = a;
        }
    }
    return true;
}

}  // namespace ccsx_pol

#endif
