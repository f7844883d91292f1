// prepare_sanitize.cpp -- drives the resumable ccs_prepare (ccsx_prep_*) and the
// pairwise aligner's seed / band split (include/ccsx_host.h) under
// AddressSanitizer + UndefinedBehaviorSanitizer on the CPU, over synthetic
// ZMWs with abnormal subreads: fused passes, truncated ones, an adapter
// read-through (a subread followed by its reverse complement), an unrelated
// read, N bases, an empty subread and two length groups.  Every walk is driven
// with both pairs of each request answered and must give ccsx_prepare's list;
// one walk in three is also begun again and abandoned while a request is
// pending, which must free everything (the leak check).
// tests/test_prepare_sanitize.py compiles it with prepare.cpp and pairwise.cpp
// alone (no HIP code is involved).
//   prepare_sanitize [ZMWs]   prints "ok <ZMWs> <requests> <abandoned>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ccsx_host.h"

static uint64_t rnd_state = 0x2545F4914F6CDD1Dull;
static uint32_t rnd(uint32_t n)
{
    rnd_state ^= rnd_state << 13, rnd_state ^= rnd_state >> 7, rnd_state ^= rnd_state << 17;
    return (uint32_t)((rnd_state >> 11) % n);
}

static std::string revcomp(std::string s)
{
    if (!s.empty()) ccsx_revcomp(&s[0], (uint32_t)s.size());
    return s;
}

static std::vector<uint8_t> codes(const std::string &s)
{
    std::vector<uint8_t> v(s.size());
    for (size_t i = 0; i < s.size(); ++i) v[i] = s[i] == 'A' ? 0 : s[i] == 'C' ? 1 : s[i] == 'G' ? 2 : s[i] == 'T' ? 3 : 4;
    return v;
}

int main(int argc, char **argv)
{
    const int nz = argc > 1 ? atoi(argv[1]) : 45;
    size_t requests = 0, abandoned = 0;
    for (int z = 0; z < nz; ++z) {
        const uint32_t L = 600 + rnd(900), passes = 5 + rnd(5);
        std::vector<char> raw((size_t)passes * (2 * L + 16) + 16);
        std::vector<uint32_t> lens(passes);
        ccsx_synth_zmw(20261020, 500000 + (uint64_t)z, L, passes, raw.data(), lens.data(), nullptr);
        std::vector<std::string> subs;
        for (size_t k = 0, o = 0; k < passes; o += lens[k], ++k) subs.emplace_back(raw.data() + o, lens[k]);
        const uint32_t i = rnd(passes);
        switch (z % 9) {
        case 1: subs[i] = subs[i].substr(0, subs[i].size() * (2 + rnd(7)) / 10); break;
        case 2: subs[i] += revcomp(subs[i]).substr(0, subs[i].size() / 2 + rnd((uint32_t)subs[i].size() / 2)); break;
        case 3: subs[i] = "ATCTCTCTCAACAACAACAACGGAGGAGGAGGAAAAGAGAGAGAT" + subs[i]; break;
        case 4:
            if (i + 1 < passes) {
                subs[i] += subs[i + 1];
                subs.erase(subs.begin() + i + 1);
            }
            break;
        case 5:
            for (char &c : subs[i]) c = "ACGT"[rnd(4)];
            break;
        case 6:
            subs[i] += subs[(i + 1) % passes];
            for (size_t k = 0; k < subs[i].size() / 50; ++k) subs[i][rnd((uint32_t)subs[i].size())] = "NnacgtRY"[rnd(8)];
            break;
        case 7: subs[i].clear(); break;
        case 8:
            // long enough for get_template_grp's head and tail checks (> 2,000 bases)
            for (size_t k = 0; k < subs.size(); k += 2) subs[k] += subs[k] + subs[k].substr(0, subs[k].size() / 3);
            break;
        default: break;
        }
        std::string seqs;
        std::vector<uint32_t> ln;
        for (const std::string &s : subs) seqs += s, ln.push_back((uint32_t)s.size());
        const uint32_t n = (uint32_t)ln.size();
        // the seed / band split on the pairs a strand check would align
        {
            const std::vector<uint8_t> t = codes(subs[0]), q = codes(subs[i % subs.size()]), q2 = codes(revcomp(subs[0]));
            for (const std::vector<uint8_t> *qq : {&q, &q2}) {
                int32_t d0 = 0;
                const ccsx_pairaln whole = ccsx_pairwise(qq->data(), (uint32_t)qq->size(), t.data(), (uint32_t)t.size());
                ccsx_pairaln parts;
                memset(&parts, 0, sizeof parts);
                if (ccsx_pairwise_seed(qq->data(), (uint32_t)qq->size(), t.data(), (uint32_t)t.size(), &d0)) {
                    parts = ccsx_pairwise_band(qq->data(), (uint32_t)qq->size(), t.data(), (uint32_t)t.size(), d0);
                    // bands that leave the target on either side
                    for (int32_t d : {d0 - 700, d0 + 700, -(int32_t)qq->size() - 300, (int32_t)t.size() + 300})
                        (void)ccsx_pairwise_band(qq->data(), (uint32_t)qq->size(), t.data(), (uint32_t)t.size(), d);
                }
                if (memcmp(&whole, &parts, sizeof whole)) return 20;
            }
            if (ccsx_pairwise_band(nullptr, 0, t.data(), (uint32_t)t.size(), 0).aln ||
                ccsx_pairwise_band(q.data(), (uint32_t)q.size(), nullptr, 0, 0).aln)
                return 21;
        }
        // the resumable walk, both pairs answered, against ccsx_prepare
        std::vector<uint32_t> o0(n + 1), l0(n + 1), o1(n + 1), l1(n + 1);
        std::vector<uint8_t> r0(n + 1), r1(n + 1);
        const uint32_t ns0 = ccsx_prepare(seqs.data(), ln.data(), n, o0.data(), l0.data(), r0.data());
        ccsx_prep *p = ccsx_prep_begin(seqs.data(), ln.data(), n);
        ccsx_pair w[2];
        uint32_t np;
        while ((np = ccsx_prep_pending(p, w)) != 0) {
            if (np != 2) return 22;
            ccsx_pairaln r[2];
            for (int k = 0; k < 2; ++k) r[k] = ccsx_pairwise(w[k].q, w[k].qlen, w[k].t, w[k].tlen);
            ccsx_prep_answer(p, r);
            ++requests;
        }
        const uint32_t ns1 = ccsx_prep_end(p, o1.data(), l1.data(), r1.data());
        if (ns0 != ns1 || memcmp(o0.data(), o1.data(), ns0 * 4) || memcmp(l0.data(), l1.data(), ns0 * 4) ||
            memcmp(r0.data(), r1.data(), ns0))
            return 23;
        for (uint32_t k = 0; k < ns1; ++k)
            if ((uint64_t)o1[k] + l1[k] > seqs.size()) return 24;
        // a walk abandoned mid-way: at its first request (even z) or after one answer
        if (z % 3 == 0) {
            ccsx_prep *a = ccsx_prep_begin(seqs.data(), ln.data(), n);
            if ((z & 1) && ccsx_prep_pending(a, w)) {
                ccsx_pairaln r[2];
                for (int k = 0; k < 2; ++k) r[k] = ccsx_pairwise(w[k].q, w[k].qlen, w[k].t, w[k].tlen);
                ccsx_prep_answer(a, r);
            }
            if (ccsx_prep_pending(a, w)) {
                ++abandoned;
                if (ccsx_prep_end(a, nullptr, nullptr, nullptr) != 0) return 25;
            } else {
                (void)ccsx_prep_end(a, o1.data(), l1.data(), r1.data());
            }
        }
    }
    // no subread at all
    ccsx_prep *e = ccsx_prep_begin("", nullptr, 0);
    ccsx_pair w[2];
    if (ccsx_prep_pending(e, w) || ccsx_prep_end(e, nullptr, nullptr, nullptr) != 0) return 26;
    printf("ok %d %zu %zu\n", nz, requests, abandoned);
    return 0;
}
