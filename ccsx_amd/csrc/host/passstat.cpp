// passstat.cpp -- host side of the per-pass alignment statistics (SPEC.md §10,
// include/ccsx_host.h): the value derived from the records the device returns.
#include "ccsx_host.h"

extern "C" {

double ccsx_pass_identity(const ccsx_pass_stat *st)
{
    if (!st) return 0.0;
    const uint64_t den = uint64_t(st->match) + st->mismatch + st->ins + st->del;
    return den ? double(st->match) / double(den) : 0.0;
}

}  // extern "C"
