// barcode.cpp -- SPEC.md §16 on the host: the barcode set's check, the scores
// of one read as a sequential loop (what ccsx_barcode.hip computes per wave;
// the same five values per end), the call from them, and the barcode file
// reader on the subread reader's record parser (ingest.cpp).
#include "ccsx_host.h"

#include <algorithm>
#include <string>
#include <vector>

#include "ccsx_barcode.h"

#ifdef CCSX_BARCODE_NO_READER
// (the stand-alone sanitizer program compiles this file alone)
#else
#include "ingest.h"
#endif

namespace {

using namespace ccsx_bc;

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

// score and end of pattern x[0 .. L) against window y[0 .. w): two columns of
// the matrix, column by column
void align(const uint8_t *x, int L, const uint8_t *y, int w, int32_t &score, int32_t &end)
{
    int32_t col[kMaxLen + 1];
    for (int i = 0; i <= L; ++i) col[i] = -kPenalty * i;
    score = col[L], end = 0;
    for (int j = 1; j <= w; ++j) {
        int32_t diag = 0;  // H(i - 1, j - 1)
        col[0] = 0;
        for (int i = 1; i <= L; ++i) {
            const int32_t left = col[i];
            const int32_t d = diag + (x[i - 1] == y[j - 1] ? kMatch : -kPenalty);
            col[i] = std::max(d, std::max(col[i - 1], left) - kPenalty);
            diag = left;
        }
        if (col[L] > score) score = col[L], end = j;
    }
}

}  // namespace

extern "C" {

int32_t ccsx_barcode_check(const char *seqs, const uint32_t *off, const uint32_t *len, uint32_t B)
{
    if (!seqs || !off || !len || B < 1 || B > kMaxSet) return -1;
    for (uint32_t b = 0; b < B; ++b) {
        if (len[b] < 1 || len[b] > kMaxLen) return -1;
        for (uint32_t k = 0; k < len[b]; ++k)
            if (!acgt(seqs[off[b] + k])) return -1;
    }
    return 0;
}

int32_t ccsx_barcode_host(const char *seqs, const uint32_t *off, const uint32_t *len, uint32_t B, uint32_t Wn,
                          const char *ccs, uint32_t n, ccsx_bc_out *out)
{
    if (Wn < 1 || Wn > kMaxWin || !out || ccsx_barcode_check(seqs, off, len, B) != 0) return -1;
    const uint32_t w = std::min(n, Wn);
    uint8_t win[2][kMaxWin], x[kMaxLen];
    for (uint32_t k = 0; k < w; ++k) {
        win[0][k] = (uint8_t)ccsx_pol::base_code((uint8_t)ccs[k]);
        win[1][k] = (uint8_t)(3u - ccsx_pol::base_code((uint8_t)ccs[n - 1 - k]));
    }
    // per end: every pattern's score and end, in pattern order
    std::vector<int32_t> sc(2 * (size_t)B), en(2 * (size_t)B);
    for (int e = 0; e < 2; ++e) {
        for (uint32_t p = 0; p < 2 * B; ++p) {
            const uint32_t b = p >> 1, L = len[b];
            const char *s = seqs + off[b];
            for (uint32_t k = 0; k < L; ++k)
                x[k] = (uint8_t)((p & 1u) ? 3u - ccsx_pol::base_code((uint8_t)s[L - 1 - k]) : ccsx_pol::base_code((uint8_t)s[k]));
            align(x, (int)L, win[e], (int)w, sc[p], en[p]);
        }
        ccsx_bc_end &r = out->e[e];
        uint32_t best = 0;
        for (uint32_t p = 1; p < 2 * B; ++p)
            if (sc[p] > sc[best]) best = p;
        r.pattern = (int32_t)best, r.score = sc[best], r.end = en[best];
        r.second = CCSX_BC_NONE, r.second_pattern = -1;
        for (uint32_t p = 0; p < 2 * B; ++p)
            if ((p >> 1) != (best >> 1) && (r.second_pattern < 0 || sc[p] > r.second)) r.second = sc[p], r.second_pattern = (int32_t)p;
    }
    return 0;
}

void ccsx_barcode_call(const ccsx_bc_out *r, const uint32_t *len, uint32_t B, uint32_t n, int32_t T, int32_t D,
                       ccsx_bc_call *call)
{
    for (int e = 0; e < 2; ++e) {
        const ccsx_bc_end &x = r->e[e];
        const int64_t L = len[(uint32_t)x.pattern >> 1];
        call->called[e] = 100 * (int64_t)x.score >= (int64_t)T * L && (B == 1 || (int64_t)x.score - x.second >= D);
    }
    call->cl = call->called[0] ? (uint32_t)r->e[0].end : 0;
    call->cr = call->called[1] ? (uint32_t)r->e[1].end : 0;
    call->reason = !call->called[0] && !call->called[1] ? CCSX_BC_NO_ENDS
                   : !call->called[0]                   ? CCSX_BC_NO_END0
                   : !call->called[1]                   ? CCSX_BC_NO_END1
                   : (uint64_t)call->cl + call->cr >= n ? CCSX_BC_NO_INSERT
                                                        : CCSX_BC_OK;
    call->assigned = call->reason == CCSX_BC_OK;
}

#ifndef CCSX_BARCODE_NO_READER
struct ccsx_barcode_set {
    std::vector<std::string> names, seqs;
    std::vector<const char *> pn, ps;
};

ccsx_barcode_set *ccsx_barcode_read(const char *path)
{
    auto src = ccsx_ingest::FxRecords::open(path);
    if (!src) return nullptr;
    auto *s = new ccsx_barcode_set();
    std::string name, bases;
    while (src->next(name, bases)) s->names.push_back(name), s->seqs.push_back(bases);
    if (s->names.empty()) {
        delete s;
        return nullptr;
    }
    for (size_t i = 0; i < s->names.size(); ++i) s->pn.push_back(s->names[i].c_str()), s->ps.push_back(s->seqs[i].c_str());
    return s;
}

uint32_t ccsx_barcode_set_get(const ccsx_barcode_set *s, const char *const **names, const char *const **seqs)
{
    if (!s) return 0;
    if (names) *names = s->pn.data();
    if (seqs) *seqs = s->ps.data();
    return (uint32_t)s->names.size();
}

void ccsx_barcode_set_free(ccsx_barcode_set *s) { delete s; }
#endif

}  // extern "C"
