// refmap.cpp -- SPEC.md §18 on the host: the reference set's check, coding and
// 13-mer index (shared with the device context, ccsx_ref.cpp), the mapping of
// one read as a sequential loop (the vote over every (target, orientation)
// pair, then ccsx_pairwise_band_path on the winner), and the report rule.
#include "ccsx_host.h"

#include <algorithm>
#include <cstring>
#include <map>
#include <numeric>
#include <vector>

#define CCSX_REF_HOST_API
#include "ccsx_polish.h"
#include "ccsx_ref.h"

namespace {

using namespace ccsx_ref;

// 0..3 for ACGT in either case, 4 for another letter, -1 for anything else
int target_code(char ch)
{
    const int lc = ch | 0x20;
    if (lc < 'a' || lc > 'z') return -1;
    switch (lc) {
    case 'a': return 0;
    case 'c': return 1;
    case 'g': return 2;
    case 't': return 3;
    default: return 4;
    }
}

}  // namespace

extern "C" {

ccsx_ref_set *ccsx_ref_set_make(const char *seqs, const uint32_t *off, const uint32_t *len, uint32_t G)
{
    if (!seqs || !off || !len || G < 1 || G > kMaxSet) return nullptr;
    uint64_t total = 0;
    for (uint32_t g = 0; g < G; ++g) {
        if (len[g] < (uint32_t)kK) return nullptr;
        total += len[g];
    }
    if (total > kMaxLetters) return nullptr;
    auto *s = new ccsx_ref_set();
    s->codes.reserve(total);
    for (uint32_t g = 0; g < G; ++g) {
        s->off.push_back((uint32_t)s->codes.size());
        s->len.push_back(len[g]);
        for (uint32_t k = 0; k < len[g]; ++k) {
            const int c = target_code(seqs[off[g] + k]);
            if (c < 0) {
                delete s;
                return nullptr;
            }
            s->codes.push_back((uint8_t)c);
        }
    }
    // every valid 13-mer as (kmer, g << 20 | pos): sorting the pairs sorts by (kmer, g, pos)
    std::vector<uint64_t> e;
    for (uint32_t g = 0; g < G; ++g) {
        const uint8_t *t = s->codes.data() + s->off[g];
        uint32_t h = 0, valid = 0;
        for (uint32_t i = 0; i < len[g]; ++i) {
            if (t[i] > 3) {
                valid = 0;
                continue;
            }
            h = ((h << 2) | t[i]) & kKmerMask;
            if (++valid >= (uint32_t)kK) e.push_back((uint64_t)h << 32 | g << kPosBits | (i + 1 - kK));
        }
    }
    std::sort(e.begin(), e.end());
    // without the k-mers that occur more than 64 times in their target
    for (size_t a = 0; a < e.size();) {
        size_t b = a;
        while (b < e.size() && (e[b] >> kPosBits) == (e[a] >> kPosBits)) ++b;
        if (b - a <= kMaxOcc)
            for (size_t k = a; k < b; ++k) s->kmer.push_back((uint32_t)(e[k] >> 32)), s->gpos.push_back((uint32_t)e[k]);
        a = b;
    }
    s->dir.assign(kDirSize, (uint32_t)s->kmer.size());
    for (size_t k = s->kmer.size(); k-- > 0;) s->dir[s->kmer[k] >> kDirShift] = (uint32_t)k;
    for (uint32_t b = kDirSize - 1; b-- > 0;) s->dir[b] = std::min(s->dir[b], s->dir[b + 1]);
    return s;
}

void ccsx_ref_set_free(ccsx_ref_set *set) { delete set; }

int32_t ccsx_ref_host(const ccsx_ref_set *set, const char *ccs, uint32_t n, ccsx_ref_rec *rec, uint32_t *words)
{
    if (!set || !rec || (n && !ccs)) return -1;
    memset(rec, 0, sizeof *rec);
    rec->g = -1;
    if (words)
        for (uint32_t i = 0; i < n; ++i) words[i] = CCSX_MAP_INS;
    std::vector<uint8_t> q[2];
    q[0].resize(n), q[1].resize(n);
    for (uint32_t i = 0; i < n; ++i) q[0][i] = (uint8_t)ccsx_pol::base_code((uint8_t)ccs[i]);
    for (uint32_t i = 0; i < n; ++i) q[1][i] = (uint8_t)(3 - q[0][n - 1 - i]);
    // the votes of every pair, by (pair, bin)
    std::map<uint32_t, uint32_t> votes;
    for (uint32_t o = 0; o < 2 && n >= (uint32_t)kK; ++o) {
        uint32_t h = 0;
        for (uint32_t i = 0; i < n; ++i) {
            h = ((h << 2) | q[o][i]) & kKmerMask;
            if (i + 1 < (uint32_t)kK) continue;
            const int64_t qp = (int64_t)i + 1 - kK;
            auto lo = std::lower_bound(set->kmer.begin(), set->kmer.end(), h);
            for (size_t k = (size_t)(lo - set->kmer.begin()); k < set->kmer.size() && set->kmer[k] == h; ++k) {
                const uint32_t g = set->gpos[k] >> kPosBits;
                const int64_t d = (int64_t)(set->gpos[k] & ((1u << kPosBits) - 1u)) - qp;
                votes[vote_key(2 * g + o, (int32_t)(d >= 0 ? d / 32 : -((-d + 31) / 32)))]++;
            }
        }
    }
    // per pair the bin with the most votes (the smallest of equals: keys ascend);
    // the winner the pair with the most (the smallest 2 g + o of equals)
    uint32_t best = 0, best_key = 0, pair_best[2 * kMaxSet] = {0};
    for (const auto &kv : votes) {
        pair_best[kv.first >> kPairShift] = std::max(pair_best[kv.first >> kPairShift], kv.second);
        if (kv.second > best) best = kv.second, best_key = kv.first;
    }
    if (!best) return 0;
    const uint32_t g = best_key >> (kPairShift + 1), o = (best_key >> kPairShift) & 1u;
    const int32_t bin = (int32_t)(best_key & ((1u << kPairShift) - 1u)) - (int32_t)kBinBias;
    uint32_t second = 0;
    for (uint32_t p = 0; p < 2 * (uint32_t)set->len.size(); ++p)
        if ((p >> 1) != g) second = std::max(second, pair_best[p]);
    const int32_t d0 = bin * 32 + 16;
    std::vector<uint32_t> w(words ? n : 0);
    const ccsx_pairaln a = ccsx_pairwise_band_path(q[o].data(), n, set->codes.data() + set->off[g], set->len[g], d0,
                                                   words ? w.data() : nullptr);
    if (!a.aln) return 0;  // (the all-zero result: unmapped)
    rec->g = (int32_t)g, rec->o = (int32_t)o, rec->d0 = d0, rec->votes = (int32_t)best, rec->votes2 = (int32_t)second;
    rec->a = a;
    if (words) std::copy(w.begin(), w.end(), words);
    return 0;
}

int32_t ccsx_ref_pass(const ccsx_ref_rec *rec, int32_t y, int32_t Y)
{
    return rec && rec->g >= 0 && rec->a.aln >= y && 100 * (int64_t)rec->a.mat >= (int64_t)Y * rec->a.aln;
}

}  // extern "C"
