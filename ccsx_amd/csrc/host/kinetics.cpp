// kinetics.cpp -- host side of the per-base consensus kinetics (SPEC.md §13,
// include/ccsx_host.h): the 8-bit codec the kernel applies (ccsx_layout.h),
// ccs_prepare with the two code planes carried along, and the SAM array tags of
// a ZMW's records.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ccsx_host.h"
#include "ccsx_layout.h"

static_assert(sizeof(ccsx_kinetics) == ccsx::kKnBytes, "ccsx_kinetics is the kernel's record");

extern "C" {

uint32_t ccsx_kin_frames(uint8_t code) { return ccsx::kin_frames(code); }

uint8_t ccsx_kin_code(uint32_t frames) { return ccsx::kin_code(frames); }

uint32_t ccsx_prepare_apply_kin(char *seqs, uint8_t *ipd, uint8_t *pw, const uint32_t *lens, uint32_t n, uint32_t *seg_off,
                                uint32_t *seg_len, uint8_t *seg_rev)
{
    std::vector<uint8_t> own;
    if (!seg_rev) {
        own.resize(n ? n : 1);
        seg_rev = own.data();
    }
    const uint32_t ns = ccsx_prepare(seqs, lens, n, seg_off, seg_len, seg_rev);
    for (uint32_t l = 0; l < ns; ++l) {
        if (!seg_rev[l]) continue;
        ccsx_revcomp(seqs + seg_off[l], seg_len[l]);
        // base j of the pushed segment is subread base len - 1 - j: its values go with it
        if (ipd) std::reverse(ipd + seg_off[l], ipd + seg_off[l] + seg_len[l]);
        if (pw) std::reverse(pw + seg_off[l], pw + seg_off[l] + seg_len[l]);
    }
    return ns;
}

long ccsx_kinetics_tags(const ccsx_kinetics *rec, uint32_t len, char *buf, size_t cap)
{
    static const char *const tag[4] = {"fi:B:C", "fp:B:C", "ri:B:C", "rp:B:C"};
    std::string s;
    s.reserve((size_t)len * 16 + 32);
    char num[8];
    for (int t = 0; t < 4; ++t) {
        if (t) s += '\t';
        s += tag[t];
        const bool rev = t >= 2;
        for (uint32_t j = 0; j < len; ++j) {
            const ccsx_kinetics &r = rec[rev ? len - 1 - j : j];
            const unsigned v = rev ? r.rev[t & 1] : r.fwd[t & 1];
            const int k = snprintf(num, sizeof num, ",%u", v);
            s.append(num, (size_t)k);
        }
    }
    if (buf && cap) {
        const size_t k = std::min(s.size(), cap - 1);
        memcpy(buf, s.data(), k);
        buf[k] = 0;
    }
    return (long)s.size();
}

}  // extern "C"
