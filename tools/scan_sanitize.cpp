// scan_sanitize.cpp -- drives ccsx_scan_host, ccsx_scan_start and ccsx_scan_cut
// (include/ccsx_host.h, SPEC.md §17) under AddressSanitizer +
// UndefinedBehaviorSanitizer on the CPU, over generated sets and reads: sets of
// 1 .. 64 adapters of 1 .. 64 letters in both cases (one adapter alone, lengths
// 1 and 64 among them), thresholds 1 .. 100 (1 and 100 among them), reads of
// 0 .. 1500 bases (0, 1 and one base short of an adapter among them) with
// adapters planted in both orientations inside most, at the first and at the
// last base among them, every buffer allocated at exactly its length; and the
// sets that are none (a letter N, lengths 0 and 65, A = 0 and 65, T = 0 and
// 101), which must be refused with the output untouched.  The hits are checked
// for their ranges, their order and the anchored maximum, the pieces for lying
// outside every hit.  tests/test_scan_host.py compiles it with host/scan.cpp
// alone (no HIP code and no input reader are involved).
//   scan_sanitize [reads]   prints "ok <reads> <hits> <refused sets>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ccsx_host.h"

static uint64_t rnd_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n)
{
    rnd_state ^= rnd_state << 13, rnd_state ^= rnd_state >> 7, rnd_state ^= rnd_state << 17;
    return (uint32_t)((rnd_state >> 11) % n);
}

static int fail(const char *what, int z)
{
    fprintf(stderr, "scan_sanitize: %s (read %d)\n", what, z);
    return 1;
}

static std::string revcomp(const std::string &s)
{
    std::string r(s.rbegin(), s.rend());
    for (auto &ch : r) ch = ch == 'A' ? 'T' : ch == 'C' ? 'G' : ch == 'G' ? 'C' : ch == 'T' ? 'A' : ch == 'a' ? 't' : ch == 'c' ? 'g' : ch == 'g' ? 'c' : 'a';
    return r;
}

int main(int argc, char **argv)
{
    const int nz = argc > 1 ? atoi(argv[1]) : 60;
    static const uint32_t small_n[] = {0, 1, 15};
    static const uint32_t edge_t[] = {1, 100, 75};
    uint64_t nhits = 0, refused = 0;
    for (int z = 0; z < nz; ++z) {
        // the set: exact-size arrays (vector<char> so that no NUL follows)
        const uint32_t A = z % 7 == 0 ? 1 : z == 8 ? 64 : 1 + rnd(12);
        std::vector<char> seqs;
        std::vector<uint32_t> off, len;
        for (uint32_t a = 0; a < A; ++a) {
            const uint32_t L = a == 0 ? (z % 3 == 0 ? 64 : 16) : a == 1 ? 1 : 8 + rnd(57);
            off.push_back((uint32_t)seqs.size());
            len.push_back(L);
            for (uint32_t k = 0; k < L; ++k) seqs.push_back("ACGTacgt"[rnd(8)]);
        }
        const uint32_t T = z < 3 ? edge_t[z] : 60 + rnd(41);
        const uint32_t n = z < 3 ? small_n[z] : rnd(1500);
        std::string read(n, 'A');
        for (auto &ch : read) ch = "ACGTNacgt"[rnd(9)];
        // most reads carry adapter 0 at the first base, a reverse complement at the last and one inside
        const bool plant = z % 4 != 3 && z >= 3;
        // (not the one-letter adapter at the end: its hit there may be suppressed by the base before)
        const uint32_t bl = rnd(A), br0 = rnd(A), br = br0 == 1 ? 0 : br0;
        if (plant) {
            const std::string a0(seqs.data() + off[0], len[0]);
            read = a0 + read + std::string(seqs.data() + off[bl], len[bl]) + read.substr(0, n / 2) +
                   revcomp(std::string(seqs.data() + off[br], len[br]));
        }
        std::vector<char> ccs(read.begin(), read.end());
        const uint32_t m = (uint32_t)ccs.size();
        const int64_t cnt = ccsx_scan_host(seqs.data(), off.data(), len.data(), A, T, ccs.data(), m, nullptr, 0);
        if (cnt < 0) return fail("a good set was refused", z);
        std::vector<ccsx_scan_hit> hits((size_t)cnt);  // exactly the counted size
        if (ccsx_scan_host(seqs.data(), off.data(), len.data(), A, T, ccs.data(), m, hits.data(), (uint64_t)cnt) != cnt)
            return fail("the second pass disagrees with the first", z);
        bool first = false, last = false;
        for (size_t k = 0; k < hits.size(); ++k) {
            const ccsx_scan_hit &h = hits[k];
            if (h.read != 0 || h.adapter >= A || h.orient > 1) return fail("hit out of range", z);
            const int32_t L = (int32_t)len[h.adapter];
            if (h.end < 1 || h.end > m || h.start >= h.end || 100 * (int64_t)h.score < (int64_t)T * L || h.score > L)
                return fail("hit's place or score out of range", z);
            if (2 * (uint64_t)(h.end - h.start) >= 3 * (uint64_t)L) return fail("a hit spans 1.5 L", z);
            if (k && (hits[k - 1].end > h.end || (hits[k - 1].end == h.end && hits[k - 1].adapter >= h.adapter)))
                return fail("hits out of order", z);
            int32_t best = 0;
            const int32_t s = ccsx_scan_start(seqs.data() + off[h.adapter], (uint32_t)L, h.orient, ccs.data(), m, h.end, &best);
            if (s != (int32_t)h.start || best != h.score) return fail("the anchored maximum is not the score", z);
            first |= h.adapter == 0 && h.start == 0 && h.score == L;
            last |= h.end == m && h.score == L;
        }
        if (plant && (!first || !last)) return fail("a planted adapter was not found", z);
        nhits += hits.size();
        // the cut: count, then fill; pieces lie outside every hit, in order
        for (uint32_t lmin : {1u, 50u}) {
            const int64_t np = ccsx_scan_cut(hits.data(), hits.size(), m, lmin, nullptr, 0);
            std::vector<ccsx_scan_piece> pc((size_t)np);
            if (ccsx_scan_cut(hits.data(), hits.size(), m, lmin, pc.data(), (uint64_t)np) != np) return fail("cut disagrees", z);
            if (hits.empty() && (np != 1 || pc[0].b != 0 || pc[0].e != m)) return fail("a read without a hit is one piece", z);
            for (size_t k = 0; k < pc.size() && !hits.empty(); ++k) {
                const ccsx_scan_piece &p = pc[k];
                if (p.b >= p.e || p.e > m || p.e - p.b < lmin || (k && pc[k - 1].e > p.b)) return fail("piece out of range", z);
                if ((p.left < 0) != (p.b == 0) || (p.right < 0) != (p.e == m) || p.left >= (int64_t)hits.size() ||
                    p.right >= (int64_t)hits.size())
                    return fail("flank out of range", z);
                if (p.left >= 0 && hits[(size_t)p.left].end != p.b) return fail("left flank does not end at the piece", z);
                if (p.right >= 0 && hits[(size_t)p.right].start != p.e) return fail("right flank does not start at the piece", z);
                for (const auto &h : hits)
                    if (h.start < p.e && p.b < h.end) return fail("a piece overlaps a hit", z);
            }
        }
        // the sets that are none: the output must stay as it is
        std::vector<ccsx_scan_hit> keep = hits;
        std::vector<char> bad = seqs;
        std::vector<uint32_t> blen = len;
        uint32_t bA = A, bT = T;
        switch (z % 7) {
        case 0: bad[rnd((uint32_t)bad.size())] = 'N'; break;
        case 1: blen[rnd(A)] = 0; break;
        case 2: blen[A - 1] = 65; break;  // (checked before any letter is read)
        case 3: bA = 0; break;
        case 4: bA = 65; break;  // (refused on its count alone)
        case 5: bT = 0; break;
        default: bT = 101; break;
        }
        if (ccsx_scan_host(bad.data(), off.data(), blen.data(), bA, bT, ccs.data(), m, hits.data(), hits.size()) != -1)
            return fail("a bad set was not refused", z);
        if (!hits.empty() && memcmp(keep.data(), hits.data(), hits.size() * sizeof(ccsx_scan_hit)) != 0)
            return fail("a refused call wrote its output", z);
        if (ccsx_scan_check(bad.data(), off.data(), blen.data(), bA, bT) == 0) return fail("check disagrees", z);
        ++refused;
    }
    printf("ok %d %llu %llu\n", nz, (unsigned long long)nhits, (unsigned long long)refused);
    return 0;
}
