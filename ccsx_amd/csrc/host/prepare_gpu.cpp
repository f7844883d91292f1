// prepare_gpu.cpp -- ccs_prepare over a chunk of ZMWs with strand_match's band
// alignments batched onto the device (ccsx_prepare_batch, include/ccsx_host.h).
//
// ccs_prepare is serial per ZMW: whether a subread is aligned depends on the
// earlier answers.  So every ZMW's walk (ccsx_prep_*, prepare.cpp) runs to its
// next request; a round seeds all the wanted pairs on the host threads
// (ccsx_pairwise_seed), runs their bands as one ccsx_gpu_band_align, and
// answers every walk; rounds repeat until no walk is pending.  A request
// carries both alignments of its decision, so a decision costs one round; the
// second one is wasted where the first is accepted (counted).
// Kept apart from prepare.cpp, which links without the device code.
#include <atomic>
#include <chrono>
#include <cstring>
#include <thread>
#include <vector>

#include "ccsx_align.h"
#include "ccsx_host.h"

namespace {

template <class F>
void on_threads(size_t n, int nthreads, F f)
{
    std::atomic<size_t> next(0);
    auto work = [&]() {
        for (size_t i; (i = next.fetch_add(1)) < n;) f(i);
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nthreads && (size_t)t < n; ++t) th.emplace_back(work);
    work();
    for (auto &t : th) t.join();
}

double now_ms()
{
    using namespace std::chrono;
    return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

}  // namespace

extern "C" int ccsx_prepare_batch(ccsx_aln_ctx *aln, const char *const *seqs, const uint32_t *const *lens,
                                  const uint32_t *n, size_t nz, int nthreads, uint32_t *const *seg_off,
                                  uint32_t *const *seg_len, uint8_t *const *seg_rev, uint32_t *nseg,
                                  ccsx_batch_info *info)
{
    const double t0 = now_ms();
    ccsx_batch_info bi;
    memset(&bi, 0, sizeof bi);
    std::vector<ccsx_prep *> prep(nz, nullptr);
    on_threads(nz, nthreads, [&](size_t i) { prep[i] = ccsx_prep_begin(seqs[i], lens[i], n[i]); });
    std::vector<size_t> open;  // the ZMWs with a request
    std::vector<ccsx_pair> want;
    ccsx_pair w[2];
    for (size_t i = 0; i < nz; ++i)
        if (ccsx_prep_pending(prep[i], w)) open.push_back(i), want.push_back(w[0]), want.push_back(w[1]);
    std::vector<int32_t> d0;
    std::vector<uint8_t> seeded;
    std::vector<ccsx_band_job> jobs;
    std::vector<ccsx_pairaln> got, res;
    std::vector<size_t> job_of;
    int rc = 0;
    while (!open.empty()) {
        const double ta = now_ms();
        const size_t np = want.size();
        d0.assign(np, 0), seeded.assign(np, 0);
        on_threads(np, nthreads, [&](size_t p) {
            seeded[p] = (uint8_t)ccsx_pairwise_seed(want[p].q, want[p].qlen, want[p].t, want[p].tlen, &d0[p]);
        });
        jobs.clear(), job_of.assign(np, (size_t)-1);
        for (size_t p = 0; p < np; ++p)
            if (seeded[p]) {
                job_of[p] = jobs.size();
                jobs.push_back(ccsx_band_job{want[p].q, want[p].t, want[p].qlen, want[p].tlen, d0[p]});
            }
        const double tb = now_ms();
        got.resize(jobs.size());
        float kms = 0;
        if (ccsx_gpu_band_align(aln, jobs.data(), jobs.size(), got.data(), &kms) != 0) {
            rc = -1;
            break;
        }
        const double tc = now_ms();
        res.resize(np);
        for (size_t p = 0; p < np; ++p) {
            if (seeded[p]) res[p] = got[job_of[p]];
            else memset(&res[p], 0, sizeof res[p]);
        }
        // answer every walk and run it to its next request
        std::vector<uint8_t> again(open.size(), 0);
        std::vector<ccsx_pair> next_want(np);
        on_threads(open.size(), nthreads, [&](size_t o) {
            ccsx_prep *p = prep[open[o]];
            ccsx_prep_answer(p, &res[2 * o]);
            again[o] = ccsx_prep_pending(p, &next_want[2 * o]) != 0;
        });
        size_t m = 0;
        for (size_t o = 0; o < open.size(); ++o)
            if (again[o]) {
                open[m] = open[o], next_want[2 * m] = next_want[2 * o], next_want[2 * m + 1] = next_want[2 * o + 1];
                ++m;
            }
        open.resize(m), next_want.resize(2 * m);
        want.swap(next_want);
        ++bi.rounds, bi.jobs += jobs.size();
        bi.seed_ms += tb - ta, bi.device_ms += tc - tb, bi.kernel_ms += kms;
    }
    uint64_t unused = 0;
    for (size_t i = 0; i < nz; ++i) unused += ccsx_prep_unused(prep[i]);
    on_threads(nz, nthreads, [&](size_t i) {
        // (after a failure the walks still pending are freed without a list)
        const uint32_t ns = ccsx_prep_end(prep[i], rc ? nullptr : seg_off[i], rc ? nullptr : seg_len[i],
                                          rc || !seg_rev ? nullptr : seg_rev[i]);
        if (!rc) nseg[i] = ns;
    });
    if (aln) ccsx_aln_count(aln, bi.rounds, unused);
    bi.total_ms = now_ms() - t0;
    if (info) *info = bi;
    return rc;
}
