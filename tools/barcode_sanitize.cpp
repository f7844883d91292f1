// barcode_sanitize.cpp -- drives ccsx_barcode_host and ccsx_barcode_call
// (include/ccsx_host.h, SPEC.md §16) under AddressSanitizer +
// UndefinedBehaviorSanitizer on the CPU, over generated sets and reads: sets of
// 1 .. 70 barcodes of 1 .. 64 letters in both cases (one barcode alone, lengths
// 1 and 64 among them), windows 1 .. 256 (1 and 256 among them), reads of
// 0 .. 700 bases (0, 1 and one base short of a barcode among them) with a
// barcode planted at either end of most, every buffer allocated at exactly its
// length; and the sets that are none (a letter N, lengths 0 and 65, B = 0 and
// 2049, windows 0 and 257), which must be refused with the output untouched.
// The values are checked for their ranges and the call for its definition.
// tests/test_barcode_host.py compiles it with host/barcode.cpp alone (no HIP
// code and no input reader are involved).
//   barcode_sanitize [reads]   prints "ok <reads> <assigned> <refused sets>"
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
    fprintf(stderr, "barcode_sanitize: %s (read %d)\n", what, z);
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
    static const uint32_t edge_w[] = {1, 256, 96};
    uint64_t assigned = 0, refused = 0;
    for (int z = 0; z < nz; ++z) {
        // the set: exact-size arrays (vector<char> so that no NUL follows)
        const uint32_t B = z % 7 == 0 ? 1 : 1 + rnd(70);
        std::vector<char> seqs;
        std::vector<uint32_t> off, len;
        for (uint32_t b = 0; b < B; ++b) {
            const uint32_t L = b == 0 ? (z % 3 == 0 ? 64 : 16) : b == 1 ? 1 : 1 + rnd(64);
            off.push_back((uint32_t)seqs.size());
            len.push_back(L);
            for (uint32_t k = 0; k < L; ++k) seqs.push_back("ACGTacgt"[rnd(8)]);
        }
        const uint32_t Wn = z < 3 ? edge_w[z] : 1 + rnd(256);
        const uint32_t n = z < 3 ? small_n[z] : rnd(700);
        std::string body(n, 'A');
        for (auto &ch : body) ch = "ACGTNacgt"[rnd(9)];
        // most reads carry barcode 0 at the start and a barcode's reverse complement at the end
        const uint32_t bl = rnd(B), br = rnd(B);
        std::string read = body;
        if (z % 4 != 3 && z >= 3)
            read = std::string(seqs.data() + off[bl], len[bl]) + body + revcomp(std::string(seqs.data() + off[br], len[br]));
        std::vector<char> ccs(read.begin(), read.end());
        ccsx_bc_out out;
        memset(&out, 0x5A, sizeof out);
        if (ccsx_barcode_host(seqs.data(), off.data(), len.data(), B, Wn, ccs.data(), (uint32_t)ccs.size(), &out) != 0)
            return fail("a good set was refused", z);
        const uint32_t w = ccs.size() < Wn ? (uint32_t)ccs.size() : Wn;
        for (int e = 0; e < 2; ++e) {
            const ccsx_bc_end &r = out.e[e];
            if (r.pattern < 0 || (uint32_t)r.pattern >= 2 * B) return fail("pattern out of range", z);
            const int32_t L = (int32_t)len[(uint32_t)r.pattern >> 1];
            if (r.score < -2 * L || r.score > L || r.end < 0 || (uint32_t)r.end > w) return fail("score or end out of range", z);
            if (B == 1 ? (r.second != CCSX_BC_NONE || r.second_pattern != -1)
                       : (r.second > r.score || r.second_pattern < 0 || (uint32_t)r.second_pattern >= 2 * B ||
                          (r.second_pattern >> 1) == (r.pattern >> 1)))
                return fail("second out of range", z);
        }
        if (z % 4 != 3 && z >= 3 && w >= len[bl] && out.e[0].score < (int32_t)len[bl])
            return fail("a planted barcode scores below its length", z);
        ccsx_bc_call call;
        ccsx_barcode_call(&out, len.data(), B, (uint32_t)ccs.size(), 60, 3, &call);
        const bool both = call.called[0] && call.called[1];
        if (call.assigned != (both && (uint64_t)call.cl + call.cr < ccs.size())) return fail("assigned against its definition", z);
        if ((call.reason == CCSX_BC_OK) != (call.assigned != 0)) return fail("reason against assigned", z);
        if (call.cl != (call.called[0] ? (uint32_t)out.e[0].end : 0) || call.cr != (call.called[1] ? (uint32_t)out.e[1].end : 0))
            return fail("clip lengths", z);
        assigned += call.assigned;
        // the sets that are none: out must stay as it is
        ccsx_bc_out keep = out;
        std::vector<char> bad = seqs;
        std::vector<uint32_t> blen = len;
        uint32_t bB = B, bW = Wn;
        switch (z % 7) {
        case 0: bad[rnd((uint32_t)bad.size())] = 'N'; break;
        case 1: blen[rnd(B)] = 0; break;
        case 2: blen[B - 1] = 65; break;  // (checked before any letter is read)
        case 3: bB = 0; break;
        case 4: bB = 2049; break;  // (refused on its count alone)
        case 5: bW = 0; break;
        default: bW = 257; break;
        }
        if (ccsx_barcode_host(bad.data(), off.data(), blen.data(), bB, bW, ccs.data(), (uint32_t)ccs.size(), &out) != -1)
            return fail("a bad set was not refused", z);
        if (memcmp(&keep, &out, sizeof out) != 0) return fail("a refused call wrote its output", z);
        if ((z % 7 < 5) != (ccsx_barcode_check(bad.data(), off.data(), blen.data(), bB) != 0)) return fail("check disagrees", z);
        ++refused;
    }
    printf("ok %d %llu %llu\n", nz, (unsigned long long)assigned, (unsigned long long)refused);
    return 0;
}
