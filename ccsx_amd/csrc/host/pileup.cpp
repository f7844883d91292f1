// pileup.cpp -- host side of the per-base strand pileup (SPEC.md §12,
// include/ccsx_host.h): the call of one strand from a record the device
// returns, by the column rule of SPEC.md §6 on that strand's counts.
#include "ccsx_host.h"
#include "ccsx_layout.h"

extern "C" {

int ccsx_pileup_call(const ccsx_pileup *p, int strand)
{
    if (!p || strand < 0 || strand > 2) return -1;
    uint32_t cnt[ccsx::kPuGap + 1];
    for (uint32_t b = 0; b <= ccsx::kPuGap; ++b)
        cnt[b] = strand == 0 ? p->fwd[b] : strand == 1 ? p->rev[b] : uint32_t(p->fwd[b]) + p->rev[b];
    uint32_t sum = 0, best = 0;
    for (uint32_t b = 0; b <= ccsx::kPuGap; ++b) sum += cnt[b];
    if (sum == 0) return -1;
    for (uint32_t b = 1; b < 4; ++b)
        if (cnt[b] > cnt[best]) best = b;
    return cnt[best] >= cnt[ccsx::kPuGap] ? int(best) : 4;
}

}  // extern "C"
