// basemap.cpp -- host side of the subread-to-CCS coordinate map (SPEC.md §11,
// include/ccsx_host.h): the alignment and CIGAR derived from the words the
// device returns for one segment.
#include <cstdio>
#include <cstring>

#include "ccsx_host.h"

namespace {

// appends to a buffer of cap bytes, counting what does not fit
struct Sink {
    char *p;
    size_t cap, n = 0;
    void put(uint64_t run, char op)
    {
        char t[24];
        const int k = snprintf(t, sizeof t, "%llu%c", (unsigned long long)run, op);
        for (int i = 0; i < k; ++i, ++n)
            if (p && n + 1 < cap) p[n] = t[i];
    }
    void end()
    {
        if (p && cap) p[n < cap ? n : cap - 1] = 0;
    }
};

}  // namespace

extern "C" {

long ccsx_map_cigar(const uint32_t *map, uint32_t len, ccsx_map_aln *aln, char *cigar, size_t cap)
{
    ccsx_map_aln a;
    memset(&a, 0, sizeof a);
    Sink out{cigar, cap};
    uint32_t qs = len, qe = 0;
    for (uint32_t j = 0; map && j < len; ++j)
        if (!(map[j] & CCSX_MAP_INS)) {
            if (qs == len) qs = j;
            qe = j + 1;
        }
    if (qs == len) {
        out.end();
        if (aln) *aln = a;
        return -1;
    }
    a.qs = qs, a.qe = qe;
    a.ts = map[qs] & CCSX_MAP_OFFSET;
    a.te = (map[qe - 1] & CCSX_MAP_OFFSET) + 1;
    char op = 0;
    uint64_t run = 0;
    auto add = [&](char o, uint64_t k) {
        if (o != op) {
            if (run) out.put(run, op);
            op = o, run = 0;
        }
        run += k;
    };
    uint32_t prev = a.ts;  // the previous aligned entry's offset
    for (uint32_t j = qs; j < qe; ++j) {
        const uint32_t w = map[j], t = w & CCSX_MAP_OFFSET;
        if (w & CCSX_MAP_INS) {
            add('I', 1), ++a.n_ins;
            continue;
        }
        if (j > qs && t > prev + 1) add('D', t - prev - 1), a.n_del += t - prev - 1;
        if (w & CCSX_MAP_MISMATCH) add('X', 1), ++a.n_x;
        else add('=', 1), ++a.n_eq;
        prev = t;
    }
    if (run) out.put(run, op);
    out.end();
    if (aln) *aln = a;
    return (long)out.n;
}

}  // extern "C"
