// quality.cpp -- host side of the per-base consensus qualities (SPEC.md §9,
// include/ccsx_host.h): the column formula the kernel applies (one definition,
// ccsx_layout.h) and the read-level predicted accuracy derived from the bytes
// the device returns.
#include <cmath>

#include "ccsx_host.h"
#include "ccsx_layout.h"

extern "C" {

uint8_t ccsx_qual_phred(uint32_t match, uint32_t cov) { return ccsx::qual_phred(match, cov); }

double ccsx_qual_rq(const uint8_t *qual, uint32_t len)
{
    if (!qual || len == 0) return 0.0;
    // a histogram of the bytes (four interleaved, so equal neighbours do not
    // wait on each other's increment), then one term per distinct quality: a
    // 30 kb read costs ~10 us on the CLI's collecting thread, where a running
    // sum of doubles (one dependent add per base) cost more than its kernel
    static const struct Perr {
        double v[256];
        Perr()
        {
            for (int q = 0; q < 256; ++q) v[q] = std::pow(10.0, -q / 10.0);
        }
    } perr;
    uint32_t h[4][256] = {};
    uint32_t i = 0;
    for (; i + 4 <= len; i += 4) ++h[0][qual[i]], ++h[1][qual[i + 1]], ++h[2][qual[i + 2]], ++h[3][qual[i + 3]];
    for (; i < len; ++i) ++h[0][qual[i]];
    double sum = 0.0;
    for (int q = 0; q < 256; ++q) sum += perr.v[q] * (double)(uint64_t(h[0][q]) + h[1][q] + h[2][q] + h[3][q]);
    return 1.0 - sum / len;
}

}  // extern "C"
