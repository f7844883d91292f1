// polish.cpp -- SPEC.md §15 as a sequential loop (include/ccsx_host.h,
// ccsx_polish_host): realign every pushed segment to the draft CCS in a
// 64-cell band guided by its §11 map, vote per draft position, emit the
// polished read.  The polisher (ccsx_polish.cpp) runs it for the ZMWs its
// arena cannot hold; the device kernels (ccsx_polish.hip) give the same bytes.
#include <vector>

#include "ccsx_host.h"
#include "ccsx_layout.h"
#include "ccsx_polish.h"

namespace {

using namespace ccsx_pol;

struct Piece {
    uint32_t first, last;  // rows
    int end_t;             // the end cell of the last row
};

// one segment: its realigned map, and its votes into the counters
void realign_segment(const uint8_t *c, uint32_t n, const uint8_t *r, uint32_t m, const uint32_t *w, uint32_t *wout,
                     std::vector<uint32_t> &cnt)
{
    std::vector<int32_t> lo(m);
    for (uint32_t i = 0; i < m; ++i) lo[i] = band_lo(w[i] & kOffset, n);
    std::vector<uint8_t> dir((size_t)m * kBand);
    std::vector<Piece> pieces;
    int32_t prev[kBand], cur[kBand];
    auto end_cell = [&](const int32_t *h) {
        int bt = 0;
        for (int t = 1; t < kBand; ++t)
            if (h[t] > h[bt]) bt = t;
        return bt;
    };
    for (uint32_t i = 0; i < m; ++i) {
        const bool first = i == 0 || lo[i] - lo[i - 1] >= kBand;
        if (first) {
            if (i) pieces.back().last = i - 1, pieces.back().end_t = end_cell(prev);
            pieces.push_back(Piece{i, i, 0});
        }
        const uint32_t rc = base_code(r[i]);
        auto P = [&](int32_t j) -> int32_t {
            if (first) return 0;
            const int32_t idx = j - lo[i - 1];
            return idx >= 0 && idx < kBand ? prev[idx] : kNeg;
        };
        for (int t = 0; t < kBand; ++t) {
            const int32_t j = lo[i] + t;
            if ((uint32_t)j >= n) {
                cur[t] = kNeg, dir[(size_t)i * kBand + t] = 0;
                continue;
            }
            int32_t v = P(j - 1) + (rc == base_code(c[j]) ? 1 : -2);
            uint8_t d = 1;
            const int32_t up = P(j) - 2, left = t ? cur[t - 1] - 2 : kNeg;
            if (up > v) v = up, d = 2;
            if (left > v) v = left, d = 3;
            cur[t] = v, dir[(size_t)i * kBand + t] = d;
        }
        for (int t = 0; t < kBand; ++t) prev[t] = cur[t];
    }
    pieces.back().last = m - 1, pieces.back().end_t = end_cell(prev);
    // traceback, last piece first, and the votes of each piece
    for (size_t p = pieces.size(); p-- > 0;) {
        const Piece &pc = pieces[p];
        int64_t i = pc.last;
        int32_t j = lo[i] + pc.end_t;
        while (i >= (int64_t)pc.first) {
            const uint8_t d = dir[(size_t)i * kBand + (j - lo[i])];
            if (d == 3) {
                --j;
            } else if (d == 2) {
                wout[i] = kIns | (uint32_t)(j + 1);
                --i;
            } else {
                wout[i] = (uint32_t)j | (base_code(r[i]) != base_code(c[j]) ? kMismatch : 0u);
                --i, --j;
            }
        }
        bool any = false;
        uint32_t f = 0, l = 0;
        for (uint32_t q = pc.first; q <= pc.last; ++q)
            if (!(wout[q] & kIns)) {
                if (!any) f = wout[q] & kOffset;
                l = wout[q] & kOffset, any = true;
            }
        if (!any) continue;
        for (uint32_t g = f; g <= l; ++g) ++cnt[(size_t)g * kCounters + kCov];
        for (uint32_t g = f + 1; g <= l; ++g) ++cnt[(size_t)g * kCounters + kCovs];
        uint32_t seen = UINT32_MAX;  // the slot of the latest insertion entry
        for (uint32_t q = pc.first; q <= pc.last; ++q) {
            const uint32_t g = wout[q] & kOffset, x = base_code(r[q]);
            if (!(wout[q] & kIns)) {
                ++cnt[(size_t)g * kCounters + kCnt + x];
            } else if (g != seen) {
                // (offsets never decrease: a slot's insertion entries are adjacent)
                seen = g;
                if (f < g && g <= l) ++cnt[(size_t)g * kCounters + kInsn], ++cnt[(size_t)g * kCounters + kInsb + x];
            }
        }
    }
}

inline uint32_t argmax4(const uint32_t *v)
{
    uint32_t b = 0;
    for (uint32_t x = 1; x < 4; ++x)
        if (v[x] > v[b]) b = x;
    return b;
}

}  // namespace

extern "C" int32_t ccsx_polish_host(const char *ccs, uint32_t n, const char *seqs, const uint32_t *seg_off,
                                    const uint32_t *seg_len, uint32_t nseg, const uint32_t *map, char *out_seq,
                                    uint8_t *out_qual, uint32_t *out_map, uint32_t *counts)
{
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    if (!map_ok(map, seg_len, nseg, n)) return CCSX_POLISH_BAD_MAP;
    uint64_t rows = 0;
    if (n == 0) {
        // nothing to align to: every base is inserted before offset 0
        for (uint32_t k = 0; k < nseg; ++k)
            for (uint32_t i = 0; i < seg_len[k]; ++i) out_map[rows++] = kIns;
        return 0;
    }
    const uint8_t *c = reinterpret_cast<const uint8_t *>(ccs);
    std::vector<uint32_t> cnt((size_t)(n + 1) * kCounters, 0u);
    for (uint32_t k = 0; k < nseg; rows += seg_len[k], ++k)
        if (seg_len[k])
            realign_segment(c, n, reinterpret_cast<const uint8_t *>(seqs) + seg_off[k], seg_len[k], map + rows,
                            out_map + rows, cnt);
    uint32_t len = 0, nsub = 0, nins = 0, ndel = 0;
    for (uint32_t g = 0; g <= n; ++g) {
        const uint32_t *v = &cnt[(size_t)g * kCounters];
        if (2 * v[kInsn] > v[kCovs]) {
            const uint32_t x = argmax4(v + kInsb);
            out_seq[len] = "ACGT"[x], out_qual[len] = ccsx::qual_phred(v[kInsb + x], v[kCovs]);
            ++len, ++nins;
        }
        if (g == n) break;
        const uint32_t cg = base_code(c[g]);
        if (v[kCov] == 0) {
            out_seq[len] = "ACGT"[cg], out_qual[len] = (uint8_t)ccsx::kQMin;
            ++len;
            continue;
        }
        const uint32_t best = argmax4(v + kCnt);
        const uint32_t gap = v[kCov] - (v[0] + v[1] + v[2] + v[3]);
        if (v[kCnt + best] >= gap) {
            out_seq[len] = "ACGT"[best], out_qual[len] = ccsx::qual_phred(v[kCnt + best], v[kCov]);
            ++len, nsub += best != cg;
        } else {
            ++ndel;
        }
    }
    counts[0] = len, counts[1] = nsub, counts[2] = nins, counts[3] = ndel;
    return 0;
}
