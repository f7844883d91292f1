// refmap_sanitize.cpp -- drives ccsx_ref_set_make, ccsx_ref_host, ccsx_ref_pass
// and ccsx_map_cigar on the words (include/ccsx_host.h, SPEC.md §18) under
// AddressSanitizer + UndefinedBehaviorSanitizer on the CPU, over generated sets
// and reads: sets of 1 .. 6 targets of 13 .. 900 letters in both cases with N
// among them (a target of exactly 13 and a tandem repeat past the 64-occurrence
// cap among them), reads of 0 .. 1200 bases (0, 12 and 13 among them) cut from
// a target in either strand with substitutions, insertions, deletions and junk
// at both ends, or random, every buffer allocated at exactly its length; and
// the sets that are none (no target, 65 targets, a target of 12 letters, a
// digit), which must be refused.  Every mapped record is checked against §18's
// identities: the words' CIGAR gives qb, qe, tb, te, mat, mis, ins, del; offsets
// never decrease; the coordinates lie inside the read and the target.
// tests/test_refmap_host.py compiles it with host/refmap.cpp, pairwise.cpp and
// basemap.cpp alone (no HIP code and no input reader are involved).
//   refmap_sanitize [reads]   prints "ok <reads> <mapped> <refused sets>"
#include <algorithm>
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
    fprintf(stderr, "refmap_sanitize: %s (read %d)\n", what, z);
    return 1;
}

static std::string revcomp(const std::string &s)
{
    std::string r(s.rbegin(), s.rend());
    for (auto &ch : r) {
        const char u = (char)(ch & ~0x20);
        ch = u == 'A' ? 'T' : u == 'C' ? 'G' : u == 'G' ? 'C' : u == 'T' ? 'A' : 'A';
    }
    return r;
}

struct Set {
    std::vector<char> seqs;
    std::vector<uint32_t> off, len;
    void add(const std::string &t) { off.push_back((uint32_t)seqs.size()), len.push_back((uint32_t)t.size()), seqs.insert(seqs.end(), t.begin(), t.end()); }
    ccsx_ref_set *make() const { return ccsx_ref_set_make(seqs.data(), off.data(), len.data(), (uint32_t)len.size()); }
};

static std::string random_target(uint32_t n)
{
    std::string t(n, 'A');
    for (auto &ch : t) ch = "ACGTacgtACGTACGTNn"[rnd(n > 40 ? 18 : 8)];
    return t;
}

int main(int argc, char **argv)
{
    const int nz = argc > 1 ? atoi(argv[1]) : 60;
    uint64_t mapped = 0, refused = 0;
    static const uint32_t small_n[] = {0, 12, 13};
    for (int z = 0; z < nz; ++z) {
        Set set;
        const uint32_t G = z % 7 == 0 ? 1 : 1 + rnd(6);
        std::vector<std::string> ts;
        for (uint32_t g = 0; g < G; ++g) {
            std::string t = g == 1 ? random_target(13) : random_target(200 + rnd(701));
            if (g == 2) {
                // a 20-base unit 70 times: its 13-mers pass the 64-occurrence cap
                const std::string u = t.substr(0, 20);
                t.clear();
                for (int k = 0; k < 70; ++k) t += u;
            }
            ts.push_back(t), set.add(t);
        }
        ccsx_ref_set *rs = set.make();
        if (!rs) return fail("a good set was refused", z);
        // the read
        std::string read;
        const uint32_t g = rnd(G);
        if (z < 3) {
            read = ts[0].substr(20, small_n[z]);
        } else if (z % 5 == 4) {
            read = random_target(50 + rnd(1000));
        } else {
            const std::string &t = ts[g];
            const uint32_t L = (uint32_t)t.size(), b = rnd(std::min(L / 2, L - 13) + 1), e = b + 13 + rnd(L - b - 12);
            for (uint32_t k = 0; k < rnd(60); ++k) read += "ACGT"[rnd(4)];
            for (uint32_t k = b; k < e && k < t.size(); ++k) {
                const uint32_t u = rnd(100);
                if (u < 3) continue;
                read += u < 6 ? "ACGT"[rnd(4)] : t[k];
                if (u >= 97) read += "ACGT"[rnd(4)];
            }
            for (uint32_t k = 0; k < rnd(60); ++k) read += "ACGT"[rnd(4)];
            if (z % 2) read = revcomp(read);
        }
        const uint32_t n = (uint32_t)read.size();
        std::vector<char> ccs(read.begin(), read.end());
        std::vector<uint32_t> words(n);
        ccsx_ref_rec rec;
        if (ccsx_ref_host(rs, ccs.data(), n, &rec, words.data()) != 0) return fail("ccsx_ref_host failed", z);
        ccsx_ref_rec rec2;
        if (ccsx_ref_host(rs, ccs.data(), n, &rec2, nullptr) != 0 || memcmp(&rec, &rec2, sizeof rec) != 0)
            return fail("the record depends on whether words are asked for", z);
        if (rec.g < 0) {
            const ccsx_ref_rec zero = {-1, 0, 0, 0, 0, {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}};
            if (memcmp(&rec, &zero, sizeof rec) != 0) return fail("an unmapped record is not all zero", z);
            for (uint32_t w : words)
                if (w != CCSX_MAP_INS) return fail("an unmapped read's word", z);
            if (ccsx_ref_pass(&rec, 0, 0)) return fail("an unmapped read passes", z);
        } else {
            ++mapped;
            const ccsx_pairaln &a = rec.a;
            if ((uint32_t)rec.g >= G || (rec.o != 0 && rec.o != 1) || rec.votes < 1 || rec.votes2 < 0 || rec.votes2 > rec.votes)
                return fail("the record's seed fields", z);
            if (a.qb < 0 || a.qb >= a.qe || (uint32_t)a.qe > n || a.tb < 0 || a.tb >= a.te || (uint32_t)a.te > set.len[(size_t)rec.g])
                return fail("the record's coordinates", z);
            ccsx_map_aln m;
            const long c = ccsx_map_cigar(words.data(), n, &m, nullptr, 0);
            std::vector<char> cg((size_t)c + 1);
            if (c < 0 || ccsx_map_cigar(words.data(), n, &m, cg.data(), cg.size()) != c) return fail("ccsx_map_cigar", z);
            if ((int32_t)m.qs != a.qb || (int32_t)m.qe != a.qe || (int32_t)m.ts != a.tb || (int32_t)m.te != a.te ||
                (int32_t)m.n_eq != a.mat || (int32_t)m.n_x != a.mis || (int32_t)m.n_ins != a.ins || (int32_t)m.n_del != a.del)
                return fail("the CIGAR of the words is not the record", z);
            uint32_t last = 0;
            for (uint32_t w : words) {
                if ((w & CCSX_MAP_OFFSET) < last) return fail("offsets decrease", z);
                last = w & CCSX_MAP_OFFSET;
            }
            if (ccsx_ref_pass(&rec, a.aln, 0) != 1 || ccsx_ref_pass(&rec, a.aln + 1, 0) != 0) return fail("ccsx_ref_pass at y", z);
        }
        ccsx_ref_set_free(rs);
        // the sets that are none
        Set none, many, shortt, digit;
        for (int k = 0; k < 65; ++k) many.add(random_target(13));
        shortt.add(ts[0]), shortt.add(random_target(12));
        std::string d = ts[0];
        d[z % d.size()] = '7';
        digit.add(d);
        for (const Set *bad : {&none, &many, &shortt, &digit}) {
            ccsx_ref_set *b = bad->make();
            if (b) return fail("a bad set was accepted", z);
            ++refused;
        }
    }
    if (ccsx_ref_host(nullptr, "ACGT", 4, nullptr, nullptr) != -1) return fail("NULL arguments", -1);
    printf("ok %d %llu %llu\n", nz, (unsigned long long)mapped, (unsigned long long)refused);
    return 0;
}
