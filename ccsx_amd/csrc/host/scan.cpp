// scan.cpp -- SPEC.md §17 on the host: the adapter set's check, the scan of one
// read as a sequential loop over one column per pattern (what ccsx_scan.hip
// computes per tile), the hit rule over the candidates, the start of a hit by
// the anchored alignment backwards from its end, and the cut of a read at its
// hits.  ccsx_scan.cpp finishes the device's candidates with the same finish().
#include "ccsx_host.h"

#include <algorithm>
#include <vector>

#define CCSX_SCAN_HOST_API
#include "ccsx_scan.h"

namespace {

using namespace ccsx_scan;

bool acgt(char ch)
{
    switch (ch | 0x20) {
    case 'a':
    case 'c':
    case 'g':
    case 't': return true;
    default: return false;
    }
}

struct Folded {
    uint32_t j, o;
    int32_t v;
};

}  // namespace

namespace ccsx_scan {

void finish(std::vector<HostCand> &c, const char *seqs, const uint32_t *off, const uint32_t *len, const ccsx_scan_in *reads,
            std::vector<ccsx_scan_hit> &out)
{
    // by (read, adapter, column, orientation); the last three as one key
    auto key = [](const HostCand &x) { return (uint64_t)(x.p >> 1) << 33 | (uint64_t)x.j << 1 | (x.p & 1u); };
    std::sort(c.begin(), c.end(),
              [&](const HostCand &x, const HostCand &y) { return x.read != y.read ? x.read < y.read : key(x) < key(y); });
    const size_t first = out.size();
    std::vector<Folded> f;
    for (size_t g0 = 0; g0 < c.size();) {
        const uint32_t read = c[g0].read, a = c[g0].p >> 1, L = len[a];
        size_t g1 = g0;
        // V_a / O_a of the group's columns: a pattern below its threshold is
        // absent and below the other
        f.clear();
        while (g1 < c.size() && c[g1].read == read && (c[g1].p >> 1) == a) {
            if (g1 + 1 < c.size() && c[g1 + 1].read == read && c[g1 + 1].p == c[g1].p + 1 && !(c[g1].p & 1u) && c[g1 + 1].j == c[g1].j) {
                const int32_t s0 = c[g1].s, s1 = c[g1 + 1].s;
                f.push_back(Folded{c[g1].j, s0 >= s1 ? 0u : 1u, std::max(s0, s1)});
                g1 += 2;
            } else {
                f.push_back(Folded{c[g1].j, c[g1].p & 1u, c[g1].s});
                g1 += 1;
            }
        }
        // the hit rule: every suppressor of a candidate is a candidate
        for (size_t x = 0; x < f.size(); ++x) {
            bool hit = true;
            for (size_t y = x; hit && y-- > 0 && f[x].j - f[y].j <= L;) hit = f[y].v < f[x].v;
            for (size_t y = x + 1; hit && y < f.size() && f[y].j - f[x].j <= L; ++y) hit = f[y].v <= f[x].v;
            if (!hit) continue;
            ccsx_scan_hit h;
            h.read = read, h.adapter = a, h.orient = f[x].o, h.end = f[x].j, h.score = f[x].v;
            h.start = (uint32_t)ccsx_scan_start(seqs + off[a], L, f[x].o, reads[read].ccs, reads[read].len, f[x].j, nullptr);
            out.push_back(h);
        }
        g0 = g1;
    }
    std::sort(out.begin() + (std::ptrdiff_t)first, out.end(), [](const ccsx_scan_hit &x, const ccsx_scan_hit &y) {
        if (x.read != y.read) return x.read < y.read;
        if (x.end != y.end) return x.end < y.end;
        return x.adapter < y.adapter;
    });
}

void candidates(const char *seqs, const uint32_t *off, const uint32_t *len, uint32_t A, uint32_t T, const char *ccs, uint32_t n,
                uint32_t read, std::vector<HostCand> &c)
{
    std::vector<uint8_t> y(n);
    for (uint32_t k = 0; k < n; ++k) y[k] = (uint8_t)ccsx_pol::base_code((uint8_t)ccs[k]);
    uint8_t x[kMaxLen];
    int32_t col[kMaxLen + 1];
    for (uint32_t p = 0; p < 2 * A; ++p) {
        const uint32_t L = len[p >> 1];
        const int32_t thr = threshold_of(L, T);
        for (uint32_t k = 0; k < L; ++k) x[k] = (uint8_t)pat_code(seqs + off[p >> 1], L, p & 1u, k);
        for (uint32_t i = 0; i <= L; ++i) col[i] = -kPenalty * (int32_t)i;
        for (uint32_t j = 1; j <= n; ++j) {
            int32_t diag = 0;  // H(i - 1, j - 1)
            col[0] = 0;
            for (uint32_t i = 1; i <= L; ++i) {
                const int32_t left = col[i];
                const int32_t d = diag + (x[i - 1] == y[j - 1] ? kMatch : -kPenalty);
                col[i] = std::max(d, std::max(col[i - 1], left) - kPenalty);
                diag = left;
            }
            if (col[L] >= thr) c.push_back(HostCand{read, p, j, col[L]});
        }
    }
}

}  // namespace ccsx_scan

extern "C" {

int32_t ccsx_scan_check(const char *seqs, const uint32_t *off, const uint32_t *len, uint32_t A, uint32_t T)
{
    if (!seqs || !off || !len || A < 1 || A > kMaxSet || T < 1 || T > 100) return -1;
    for (uint32_t a = 0; a < A; ++a) {
        if (len[a] < 1 || len[a] > kMaxLen) return -1;
        for (uint32_t k = 0; k < len[a]; ++k)
            if (!acgt(seqs[off[a] + k])) return -1;
    }
    return 0;
}

int32_t ccsx_scan_start(const char *adapter, uint32_t L, uint32_t orient, const char *ccs, uint32_t n, uint32_t end,
                        int32_t *score)
{
    if (!adapter || L < 1 || L > kMaxLen || end > n || (end && !ccs)) return -1;
    const uint32_t K = std::min(end, 2 * L);
    uint8_t x[kMaxLen];  // the pattern reversed
    for (uint32_t k = 0; k < L; ++k) x[k] = (uint8_t)pat_code(adapter, L, orient ? 1u : 0u, L - 1 - k);
    int32_t col[kMaxLen + 1];
    for (uint32_t i = 0; i <= L; ++i) col[i] = -kPenalty * (int32_t)i;
    int32_t best = col[L];
    uint32_t bestk = 0;
    for (uint32_t k = 1; k <= K; ++k) {
        const uint8_t y = (uint8_t)ccsx_pol::base_code((uint8_t)ccs[end - k]);
        int32_t diag = col[0];  // G(i - 1, k - 1)
        col[0] = -kPenalty * (int32_t)k;
        for (uint32_t i = 1; i <= L; ++i) {
            const int32_t left = col[i];
            const int32_t d = diag + (x[i - 1] == y ? kMatch : -kPenalty);
            col[i] = std::max(d, std::max(col[i - 1], left) - kPenalty);
            diag = left;
        }
        if (col[L] > best) best = col[L], bestk = k;
    }
    if (score) *score = best;
    return (int32_t)(end - bestk);
}

int64_t ccsx_scan_host(const char *seqs, const uint32_t *off, const uint32_t *len, uint32_t A, uint32_t T, const char *ccs,
                       uint32_t n, ccsx_scan_hit *hits, uint64_t cap)
{
    if (ccsx_scan_check(seqs, off, len, A, T) != 0 || (n && !ccs)) return -1;
    std::vector<HostCand> c;
    candidates(seqs, off, len, A, T, ccs, n, 0, c);
    const ccsx_scan_in in{ccs, n};
    std::vector<ccsx_scan_hit> out;
    finish(c, seqs, off, len, &in, out);
    if (hits)
        for (uint64_t k = 0; k < out.size() && k < cap; ++k) hits[k] = out[k];
    return (int64_t)out.size();
}

int64_t ccsx_scan_cut(const ccsx_scan_hit *hits, uint64_t nhits, uint32_t n, uint32_t Lmin, ccsx_scan_piece *pieces,
                      uint64_t cap)
{
    uint64_t np = 0;
    auto put = [&](uint32_t b, uint32_t e, int32_t left, int32_t right) {
        if (pieces && np < cap) pieces[np] = ccsx_scan_piece{b, e, left, right};
        ++np;
    };
    if (!nhits || !hits) {
        put(0, n, -1, -1);
        return (int64_t)np;
    }
    const uint32_t lmin = std::max(Lmin, 1u);
    std::vector<uint32_t> ord((size_t)nhits);
    for (uint64_t k = 0; k < nhits; ++k) ord[(size_t)k] = (uint32_t)k;
    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) { return hits[x].start < hits[y].start; });
    uint32_t b = 0;     // the piece under way starts here ...
    int32_t left = -1;  // ... after this hit
    for (size_t k = 0; k < ord.size();) {
        // the merged interval [ms, me) from ord[k] on; its first hit in list
        // order with start = ms, and with end = me
        const uint32_t ms = hits[ord[k]].start;
        uint32_t me = hits[ord[k]].end;
        int32_t first = (int32_t)ord[k], last = (int32_t)ord[k];
        for (++k; k < ord.size() && hits[ord[k]].start <= me; ++k) {
            const ccsx_scan_hit &h = hits[ord[k]];
            if (h.start == ms && (int32_t)ord[k] < first) first = (int32_t)ord[k];
            if (h.end > me || (h.end == me && (int32_t)ord[k] < last)) me = h.end, last = (int32_t)ord[k];
        }
        if (ms > b && ms - b >= lmin) put(b, ms, left, first);
        b = me, left = last;
    }
    if (n > b && n - b >= lmin) put(b, n, left, -1);
    return (int64_t)np;
}

}  // extern "C"
