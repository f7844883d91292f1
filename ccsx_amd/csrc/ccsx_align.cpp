// ccsx_align.cpp -- host side of the band aligner (include/ccsx_gpu.h,
// ccsx_gpu_aln_* / ccsx_gpu_band_align; the kernel is ccsx_align.hip).
//
// An aligner context owns one stream, one device arena (at most max_bytes,
// allocated at the first job and grown as slices need) and two pinned staging
// buffers.  ccsx_gpu_band_align cuts its jobs, in order, into slices that fit
// the arena; a slice is, from the arena's start: the job table, the results
// (ten words per job), the jobs' q and t bytes, and the traceback records
// (256 bytes per query row, ccsx_align.h).  Per slice: one copy in, one
// launch, one copy out.  A job that no arena of max_bytes holds, or whose
// coordinates pass the kernel's range, runs ccsx_pairwise_band here.
#include "ccsx_gpu.h"
#include "ccsx_host.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "ccsx_align.h"

extern "C" hipError_t ccsx_launch_band_align(const ccsx_aln::Args *a, uint32_t blocks, hipStream_t s);

struct ccsx_aln_ctx {
    int device = 0;
    uint64_t max_bytes = 0;
    uint32_t ncu = 256;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    uint8_t *arena = nullptr;
    uint64_t arena_bytes = 0;
    uint8_t *h_in = nullptr, *h_out = nullptr;  // pinned staging
    uint64_t h_in_bytes = 0, h_out_bytes = 0;
    uint64_t stats[5] = {0, 0, 0, 0, 0};
    std::string err;
    std::mutex mu;
};

namespace {

using namespace ccsx_aln;

constexpr uint64_t kDefaultBytes = 4ull << 30;
constexpr uint64_t kAlign = 256;

inline uint64_t up(uint64_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

// the bytes of a slice of n jobs with `seq` sequence bytes and `rows` query rows
inline uint64_t slice_bytes(uint64_t n, uint64_t seq, uint64_t rows)
{
    return up(n * sizeof(Job)) + up(n * sizeof(ccsx_pairaln)) + up(seq) + rows * kRowBytes;
}

inline uint64_t seq_bytes(const ccsx_band_job &j) { return (uint64_t)j.qlen + j.tlen; }

bool fail(ccsx_aln_ctx *c, const char *what, hipError_t e)
{
    c->err = std::string(what) + ": " + hipGetErrorString(e);
    return false;
}

bool grow_pinned(ccsx_aln_ctx *c, uint8_t *&p, uint64_t &have, uint64_t need)
{
    if (need <= have) return true;
    if (p) (void)hipHostFree(p);
    p = nullptr, have = 0;
    need = std::max<uint64_t>(need + need / 4, 1u << 20);
    const hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&p), need, hipHostMallocDefault);
    if (e != hipSuccess) return fail(c, "hipHostMalloc (aligner staging)", e);
    have = need;
    return true;
}

bool grow_arena(ccsx_aln_ctx *c, uint64_t need)
{
    if (need <= c->arena_bytes) return true;
    if (c->arena) (void)hipFree(c->arena);
    c->arena = nullptr, c->arena_bytes = 0;
    // in steps of 64 MiB, a quarter ahead, never past max_bytes
    const uint64_t step = 64ull << 20;
    need = std::min<uint64_t>(c->max_bytes, (need + need / 4 + step - 1) / step * step);
    const hipError_t e = hipMalloc(reinterpret_cast<void **>(&c->arena), need);
    if (e != hipSuccess) return fail(c, "hipMalloc (aligner arena)", e);
    c->arena_bytes = need;
    return true;
}

// jobs[idx[0 .. n)] as one slice
bool run_slice(ccsx_aln_ctx *c, const ccsx_band_job *jobs, const size_t *idx, size_t n, uint64_t seq, uint64_t rows,
               ccsx_pairaln *out, float *kernel_ms)
{
    const uint64_t o_out = up(n * sizeof(Job)), o_seq = o_out + up(n * sizeof(ccsx_pairaln)), o_rec = o_seq + up(seq);
    if (!grow_arena(c, o_rec + rows * kRowBytes) || !grow_pinned(c, c->h_in, c->h_in_bytes, o_seq + seq) ||
        !grow_pinned(c, c->h_out, c->h_out_bytes, n * sizeof(ccsx_pairaln)))
        return false;
    Job *tab = reinterpret_cast<Job *>(c->h_in);
    uint64_t so = 0, ro = 0;
    for (size_t s = 0; s < n; ++s) {
        const ccsx_band_job &j = jobs[idx[s]];
        tab[s] = Job{so, so + j.qlen, ro, j.qlen, j.tlen, j.d0, 0u};
        if (j.qlen) memcpy(c->h_in + o_seq + so, j.q, j.qlen);
        if (j.tlen) memcpy(c->h_in + o_seq + so + j.qlen, j.t, j.tlen);
        so += seq_bytes(j);
        ro += (uint64_t)j.qlen * kRowWords;
    }
    // (the gap between the tables and the sequences is copied as it is)
    hipError_t e = hipMemcpyAsync(c->arena, c->h_in, o_seq + seq, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return fail(c, "hipMemcpyAsync (aligner in)", e);
    Args a;
    a.jobs = reinterpret_cast<const Job *>(c->arena);
    a.out = reinterpret_cast<int32_t *>(c->arena + o_out);
    a.seq = c->arena + o_seq;
    a.rec = reinterpret_cast<uint32_t *>(c->arena + o_rec);
    a.njobs = (uint32_t)n;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(n, (uint64_t)c->ncu * 8u);
    if ((e = hipEventRecord(c->ev0, c->stream)) != hipSuccess) return fail(c, "hipEventRecord", e);
    if ((e = ccsx_launch_band_align(&a, blocks, c->stream)) != hipSuccess) return fail(c, "band_align launch", e);
    if ((e = hipEventRecord(c->ev1, c->stream)) != hipSuccess) return fail(c, "hipEventRecord", e);
    e = hipMemcpyAsync(c->h_out, c->arena + o_out, n * sizeof(ccsx_pairaln), hipMemcpyDeviceToHost, c->stream);
    if (e != hipSuccess) return fail(c, "hipMemcpyAsync (aligner out)", e);
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return fail(c, "band_align", e);
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->ev0, c->ev1) == hipSuccess && kernel_ms) *kernel_ms += ms;
    const ccsx_pairaln *r = reinterpret_cast<const ccsx_pairaln *>(c->h_out);
    for (size_t s = 0; s < n; ++s) out[idx[s]] = r[s];
    ++c->stats[1];
    return true;
}

}  // namespace

// ccsx_prepare_batch's counters (host/prepare_gpu.cpp)
void ccsx_aln_count(ccsx_aln_ctx *c, uint64_t rounds, uint64_t discarded)
{
    std::lock_guard<std::mutex> g(c->mu);
    c->stats[3] += rounds, c->stats[4] += discarded;
}

extern "C" {

int ccsx_gpu_aln_open(int device, uint64_t max_bytes, ccsx_aln_ctx **out)
{
    *out = nullptr;
    auto *c = new ccsx_aln_ctx();
    c->device = device;
    c->max_bytes = max_bytes ? max_bytes : kDefaultBytes;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&c->ev0);
    if (e == hipSuccess) e = hipEventCreate(&c->ev1);
    if (e != hipSuccess) {
        fprintf(stderr, "[ccsx_gpu] cannot open an aligner on device %d: %s\n", device, hipGetErrorString(e));
        ccsx_gpu_aln_close(c);
        return -1;
    }
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && n > 0) c->ncu = (uint32_t)n;
    *out = c;
    return 0;
}

void ccsx_gpu_aln_close(ccsx_aln_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->arena) (void)hipFree(c->arena);
    if (c->h_in) (void)hipHostFree(c->h_in);
    if (c->h_out) (void)hipHostFree(c->h_out);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char *ccsx_gpu_aln_error(const ccsx_aln_ctx *c) { return c ? c->err.c_str() : "no context"; }

int ccsx_gpu_band_align(ccsx_aln_ctx *c, const ccsx_band_job *jobs, size_t n, ccsx_pairaln *out, float *kernel_ms)
{
    if (!c) return -1;
    std::lock_guard<std::mutex> g(c->mu);
    if (kernel_ms) *kernel_ms = 0;
    if (n == 0) return 0;
    if (!jobs || !out) {
        c->err = "ccsx_gpu_band_align: null argument";
        return -1;
    }
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) {
        fail(c, "hipSetDevice", e);
        return -1;
    }
    c->stats[0] += n;
    std::vector<size_t> idx;
    uint64_t seq = 0, rows = 0;
    auto flush = [&]() {
        const bool ok = idx.empty() || run_slice(c, jobs, idx.data(), idx.size(), seq, rows, out, kernel_ms);
        idx.clear(), seq = rows = 0;
        return ok;
    };
    for (size_t i = 0; i < n; ++i) {
        const ccsx_band_job &j = jobs[i];
        const int64_t d0 = j.d0;
        if (j.qlen >= kMaxLen || j.tlen >= kMaxLen || d0 >= (int64_t)kMaxLen || d0 <= -(int64_t)kMaxLen ||
            slice_bytes(1, seq_bytes(j), j.qlen) > c->max_bytes) {
            out[i] = ccsx_pairwise_band(j.q, j.qlen, j.t, j.tlen, j.d0);
            ++c->stats[2];
            continue;
        }
        if (slice_bytes(idx.size() + 1, seq + seq_bytes(j), rows + j.qlen) > c->max_bytes && !flush()) return -1;
        idx.push_back(i);
        seq += seq_bytes(j), rows += j.qlen;
    }
    return flush() ? 0 : -1;
}

int ccsx_gpu_aln_stats(const ccsx_aln_ctx *c, uint64_t *stats, uint32_t n)
{
    if (!c || !stats) return -1;
    for (uint32_t i = 0; i < n && i < 5; ++i) stats[i] = c->stats[i];
    return 0;
}

}  // extern "C"
