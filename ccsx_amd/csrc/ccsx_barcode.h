// ccsx_barcode.h -- what the demultiplexer's kernel (ccsx_barcode.hip), its
// host side (ccsx_barcode.cpp) and the host restatement (host/barcode.cpp)
// share: SPEC.md §16's constants, the pattern table, the slice layout in the
// demultiplexer's arena and the launcher.  DESIGN.md §20 describes the layout.
#ifndef CCSX_BARCODE_H
#define CCSX_BARCODE_H
#include <stdint.h>

#include "ccsx_polish.h"  // ccsx_pol::base_code (SPEC.md §1's coding)

namespace ccsx_bc {

constexpr uint32_t kMaxSet = 2048;   // B
constexpr uint32_t kMaxLen = 64;     // L_b
constexpr uint32_t kMaxWin = 256;    // Wn
constexpr uint32_t kDefWin = 96;
constexpr int32_t kNone = INT32_MIN;  // CCSX_BC_NONE
constexpr int kMatch = 1, kPenalty = 2;  // s = +1 / -2, gaps -2
// a pattern's key in the reductions: (score + kBias) << kKeyBits | (kKeyMask - p).
// score >= -2 L >= -128 and p < 2 B <= 4096, so a key is positive, the largest
// key is the largest score and, among equal scores, the smallest p; 0 = none
constexpr int kBias = 1024, kKeyBits = 12, kKeyMask = (1 << kKeyBits) - 1;
constexpr uint32_t kLanes = 64;      // patterns per chunk: one per lane

// One pattern for the kernel, right-aligned in LR rows (LR = the set's longest
// barcode rounded up to 16): base k of its L bases is row LR - L + 1 + k, and
// bit (row - 1) of p0 / p1 holds bit 0 / 1 of that base's code.  act has the
// bits of its L rows.  The rows above are the definition's row 0 again (H = 0),
// so every lane's score is in the last row whatever its length.  len = 0: a
// padding lane of the last chunk.
struct Pat {
    uint64_t p0, p1, act;
    int32_t len, pad;
};

// the rows the kernel runs for a set whose longest barcode has maxlen bases
inline uint32_t rows_of(uint32_t maxlen) { return (maxlen + 15u) / 16u * 16u; }

// pattern p = 2 b + o of barcode x[0 .. L) (ASCII ACGT in either case, checked
// by the caller) in LR rows
inline Pat make_pat(const char *x, uint32_t L, uint32_t o, uint32_t LR)
{
    Pat t{0, 0, 0, (int32_t)L, 0};
    const uint32_t skip = LR - L;
    for (uint32_t k = 0; k < L; ++k) {
        const uint32_t c = o ? 3u - ccsx_pol::base_code((uint8_t)x[L - 1 - k]) : ccsx_pol::base_code((uint8_t)x[k]);
        t.p0 |= (uint64_t)(c & 1u) << (skip + k);
        t.p1 |= (uint64_t)(c >> 1) << (skip + k);
        t.act |= 1ull << (skip + k);
    }
    return t;
}

// A slice of the arena, from its start: the windows (two per ZMW, wn bytes
// each, codes 0..3: end 0 then end 1, both read from the outside inwards), the
// window length w per ZMW, then the result: five words per (ZMW, end).
struct Args {
    const Pat *pats;       // nchunks * 64 patterns (the set: uploaded by ccsx_gpu_bc_set)
    const uint8_t *win;    // job j = 2 z + e at win + j * wn
    const uint32_t *wlen;  // per ZMW
    int32_t *out;          // per job: pattern, score, end, second, second_pattern
    uint32_t njobs, nchunks, wn;
};

}  // namespace ccsx_bc

#endif
