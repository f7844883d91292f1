// polish_sanitize.cpp -- drives ccsx_polish_host (include/ccsx_host.h, SPEC.md
// §15) under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU, over
// synthetic ZMWs: drafts of 0 .. 3,000 bases (0, 1, 63, 64 and 65 among them),
// noisy segments with the anchors a POA would give, empty segments, segments
// that skip more than a band of the draft (several pieces), and, every fourth
// ZMW, a bad map (a decreasing anchor or one past the draft).  The outputs are
// allocated at exactly their documented sizes, and §11's invariants are checked
// on every realigned map.  tests/test_polish_host.py compiles it with
// host/polish.cpp alone (no HIP code is involved).
//   polish_sanitize [ZMWs]   prints "ok <ZMWs> <bad maps> <piece breaks>"
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "ccsx_host.h"

static uint64_t rnd_state = 0x2545F4914F6CDD1Dull;
static uint32_t rnd(uint32_t n)
{
    rnd_state ^= rnd_state << 13, rnd_state ^= rnd_state >> 7, rnd_state ^= rnd_state << 17;
    return (uint32_t)((rnd_state >> 11) % n);
}

static int fail(const char *what, int z)
{
    fprintf(stderr, "polish_sanitize: %s (ZMW %d)\n", what, z);
    return 1;
}

int main(int argc, char **argv)
{
    const int nz = argc > 1 ? atoi(argv[1]) : 40;
    static const uint32_t small[] = {0, 1, 63, 64, 65};
    uint64_t bad = 0, breaks = 0;
    for (int z = 0; z < nz; ++z) {
        const uint32_t n = z < 5 ? small[z] : 100 + rnd(2900);
        std::string ccs(n, 'A');
        for (auto &ch : ccs) ch = "ACGT"[rnd(4)];
        std::string seqs;
        std::vector<uint32_t> off, len, map;
        const uint32_t nseg = 1 + rnd(8);
        for (uint32_t k = 0; k < nseg; ++k) {
            off.push_back((uint32_t)seqs.size());
            const size_t at = seqs.size();
            if (k == 0 || rnd(6) != 0) {
                uint32_t p = n ? rnd(n) / 2 : 0;
                const uint32_t end = n ? p + rnd(n - p) + 1 : 0;
                for (; p < end; ++p) {
                    if (rnd(200) == 0) {
                        // skip far enough for a piece break
                        p += 64 + rnd(400);
                        if (p >= end) break;
                        ++breaks;
                    }
                    const uint32_t r = rnd(100);
                    if (r < 4) continue;
                    seqs.push_back(r < 6 ? "ACGT"[rnd(4)] : ccs[p]);
                    map.push_back(p);
                    while (rnd(100) < 4) seqs.push_back("ACGTn"[rnd(5)]), map.push_back(CCSX_MAP_INS | (p + 1));
                }
            }
            len.push_back((uint32_t)(seqs.size() - at));
        }
        const bool make_bad = z % 4 == 3 && !map.empty();
        if (make_bad) {
            const size_t i = rnd((uint32_t)map.size());
            // (a single base's anchor past the draft, or one below its predecessor's)
            if (rnd(2) || i == 0 || (map[i - 1] & CCSX_MAP_OFFSET) == 0) map[i] = n + 1;
            else map[i] = (map[i - 1] & CCSX_MAP_OFFSET) - 1, map[i - 1] &= CCSX_MAP_OFFSET;
            // the changed word must not start a segment, where a smaller anchor is no decrease
            size_t o = 0;
            for (uint32_t k = 0; k < nseg; o += len[k], ++k)
                if (o == i) map[i] = n + 1;
        }
        std::vector<char> oseq(2 * (size_t)n + 1);
        std::vector<uint8_t> oqual(2 * (size_t)n + 1);
        std::vector<uint32_t> omap(map.size());  // (exactly one word per base: data() may be null)
        uint32_t counts[4];
        const int32_t st = ccsx_polish_host(ccs.data(), n, seqs.data(), off.data(), len.data(), nseg, map.data(), oseq.data(),
                                            oqual.data(), omap.data(), counts);
        if (make_bad) {
            if (st != CCSX_POLISH_BAD_MAP || counts[0]) return fail("a bad map was not refused", z);
            ++bad;
            continue;
        }
        if (st != 0) return fail("a good map was refused", z);
        if (counts[0] > 2 * (size_t)n + 1 || counts[0] + counts[3] != n + counts[2]) return fail("counts do not add up", z);
        size_t o = 0;
        for (uint32_t k = 0; k < nseg; o += len[k], ++k) {
            uint32_t prev = 0, prev_al = 0;
            bool any_al = false;
            for (uint32_t i = 0; i < len[k]; ++i) {
                const uint32_t w = omap[o + i], t = w & CCSX_MAP_OFFSET;
                const bool ins = (w & CCSX_MAP_INS) != 0;
                if (ins && (w & CCSX_MAP_MISMATCH)) return fail("both flags", z);
                if (t < prev || t > n || (!ins && t >= n)) return fail("offset out of order or range", z);
                if (!ins && any_al && t <= prev_al) return fail("aligned offsets do not increase", z);
                prev = t;
                if (!ins) prev_al = t, any_al = true;
            }
        }
    }
    printf("ok %d %llu %llu\n", nz, (unsigned long long)bad, (unsigned long long)breaks);
    return 0;
}
