// ccsx_ref.cpp -- host side of the reference mapper (include/ccsx_gpu.h,
// ccsx_gpu_ref_*; the kernels are ccsx_ref.hip's vote and ccsx_align.hip's
// band with path).
//
// A mapper context owns one stream, one device arena (at most max_bytes,
// allocated at the first call and grown as slices need) and two pinned staging
// buffers.  The arena's head is the current set (target codes, per-target
// offset and length, the sorted 13-mer table and its directory), uploaded again
// whenever the arena or the set changes.  ccsx_gpu_ref_map cuts its reads, in
// order, into slices that fit behind the head; a slice is: what goes in (the
// band jobs with their record and word offsets, the read table, the reads'
// codes), the reverse complements, what comes out (the votes, the band's ten
// words per read, the path words) and the traceback records (256 bytes per
// base, ccsx_align.h).  Per slice: one copy in, the vote kernel, the band
// kernel on the jobs the vote kernel finished, one copy out; nothing comes to
// the host in between.  A read of 2^27 bases or more, one that no arena of
// max_bytes holds and one the vote kernel flagged run ccsx_ref_host here.
#include "ccsx_gpu.h"
#include "ccsx_host.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#define CCSX_REF_HOST_API
#include "ccsx_polish.h"
#include "ccsx_ref.h"

extern "C" hipError_t ccsx_launch_ref_vote(const ccsx_ref::Args *a, uint32_t blocks, hipStream_t s);
extern "C" hipError_t ccsx_launch_band_align_path(const ccsx_aln::PathArgs *a, uint32_t blocks, hipStream_t s);

struct ccsx_ref_ctx {
    int device = 0;
    uint64_t max_bytes = 0;
    uint32_t ncu = 256, slots = ccsx_ref::kVoteSlots;
    hipStream_t stream = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    ccsx_ref_set set;         // the current set (a copy); empty: none
    bool set_on_device = false;
    uint8_t *arena = nullptr;
    uint64_t arena_bytes = 0;
    uint8_t *h_in = nullptr, *h_out = nullptr;  // pinned staging
    uint64_t h_in_bytes = 0, h_out_bytes = 0;
    uint64_t stats[6] = {0, 0, 0, 0, 0, 0};
    std::string err;
    std::mutex mu;
};

namespace {

using namespace ccsx_ref;
using ccsx_aln::Job;
using ccsx_aln::kRowBytes;
using ccsx_aln::kRowWords;

constexpr uint64_t kDefaultBytes = 4ull << 30;
constexpr uint64_t kAlign = 256;

inline uint64_t up(uint64_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

struct CodeTable {
    uint8_t c[256];
    CodeTable()
    {
        for (int ch = 0; ch < 256; ++ch) c[ch] = (uint8_t)ccsx_pol::base_code((uint8_t)ch);
    }
};
const CodeTable kCode;

// the set's parts from the arena's start
struct Head {
    uint64_t codes, toff, tlen, kmer, gpos, dir, end;
    explicit Head(const ccsx_ref_set &s)
    {
        codes = 0;
        toff = up(s.codes.size());
        tlen = toff + up(kMaxSet * 4);
        kmer = tlen + up(kMaxSet * 4);
        gpos = kmer + up(s.kmer.size() * 4);
        dir = gpos + up(s.gpos.size() * 4);
        end = dir + up((uint64_t)kDirSize * 4);
    }
};

// a slice of nr reads with `bases` bases in all, from the head's end
struct Layout {
    uint64_t jobs, reads, fwd, in_end, rc, votes, out, words, out_end, rec, end;
    Layout(uint64_t base, uint64_t nr, uint64_t bases)
    {
        jobs = base;
        reads = jobs + up(nr * sizeof(Job));
        fwd = reads + up(nr * sizeof(Read));
        in_end = fwd + up(bases);
        rc = in_end;
        votes = rc + up(bases);
        out = votes + up(nr * sizeof(Vote));
        words = out + up(nr * sizeof(ccsx_pairaln));
        out_end = words + up(bases * 4);
        rec = out_end;
        end = rec + bases * kRowBytes;
    }
};

bool fail(ccsx_ref_ctx *c, const char *what, hipError_t e)
{
    c->err = std::string(what) + ": " + hipGetErrorString(e);
    return false;
}

bool grow_pinned(ccsx_ref_ctx *c, uint8_t *&p, uint64_t &have, uint64_t need)
{
    if (need <= have) return true;
    if (p) (void)hipHostFree(p);
    p = nullptr, have = 0;
    need = std::max<uint64_t>(need + need / 4, 1u << 20);
    const hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&p), need, hipHostMallocDefault);
    if (e != hipSuccess) return fail(c, "hipHostMalloc (mapper staging)", e);
    have = need;
    return true;
}

bool grow_arena(ccsx_ref_ctx *c, uint64_t need)
{
    if (need <= c->arena_bytes) return true;
    if (c->arena) (void)hipFree(c->arena);
    c->arena = nullptr, c->arena_bytes = 0, c->set_on_device = false;
    // in steps of 64 MiB, a quarter ahead, never past max_bytes (nor below the need)
    const uint64_t step = 64ull << 20;
    need = std::max(need, std::min<uint64_t>(c->max_bytes, (need + need / 4 + step - 1) / step * step));
    const hipError_t e = hipMalloc(reinterpret_cast<void **>(&c->arena), need);
    if (e != hipSuccess) return fail(c, "hipMalloc (mapper arena)", e);
    c->arena_bytes = need;
    return true;
}

// the set into the arena's head
bool upload_set(ccsx_ref_ctx *c)
{
    if (c->set_on_device) return true;
    const ccsx_ref_set &s = c->set;
    const Head H(s);
    if (!grow_pinned(c, c->h_in, c->h_in_bytes, H.end)) return false;
    memset(c->h_in, 0, H.end);
    memcpy(c->h_in + H.codes, s.codes.data(), s.codes.size());
    // (a target's offset is what a band job takes: bytes from the arena's start)
    memcpy(c->h_in + H.toff, s.off.data(), s.off.size() * 4);
    memcpy(c->h_in + H.tlen, s.len.data(), s.len.size() * 4);
    if (!s.kmer.empty()) {
        memcpy(c->h_in + H.kmer, s.kmer.data(), s.kmer.size() * 4);
        memcpy(c->h_in + H.gpos, s.gpos.data(), s.gpos.size() * 4);
    }
    memcpy(c->h_in + H.dir, s.dir.data(), s.dir.size() * 4);
    hipError_t e = hipMemcpyAsync(c->arena, c->h_in, H.end, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, "hipMemcpyAsync (mapper set)", e);
    c->set_on_device = true;
    return true;
}

void host_read(ccsx_ref_ctx *c, const ccsx_scan_in &z, ccsx_ref_rec *rec, uint32_t *words)
{
    (void)ccsx_ref_host(&c->set, z.ccs, z.len, rec, words);
    ++c->stats[5];
}

// z[lo .. hi) as one slice; woff[r] = read r's first word in `words`
bool run_slice(ccsx_ref_ctx *c, const ccsx_scan_in *z, size_t lo, size_t hi, uint64_t bases, const uint64_t *woff,
               ccsx_ref_rec *recs, uint32_t *words, float *kernel_ms)
{
    const size_t nr = hi - lo;
    const Head H(c->set);
    const Layout L(H.end, nr, bases);
    if (!grow_arena(c, L.end) || !upload_set(c) || !grow_pinned(c, c->h_in, c->h_in_bytes, L.in_end - L.jobs) ||
        !grow_pinned(c, c->h_out, c->h_out_bytes, L.out_end - L.votes))
        return false;
    // (the staging buffers mirror the arena from L.jobs and from L.votes on)
    Job *jobs = reinterpret_cast<Job *>(c->h_in);
    Read *reads = reinterpret_cast<Read *>(c->h_in + (L.reads - L.jobs));
    uint64_t at = 0;
    for (size_t r = 0; r < nr; ++r) {
        const uint32_t n = z[lo + r].len;
        const uint8_t *q = reinterpret_cast<const uint8_t *>(z[lo + r].ccs);
        uint8_t *t = c->h_in + (L.fwd - L.jobs) + at;
        for (uint32_t b = 0; b < n; ++b) t[b] = kCode.c[q[b]];
        reads[r] = Read{L.fwd + at, L.rc + at, n, 0u};
        // the record and word space of the read, reserved whatever the vote gives
        jobs[r] = Job{0, 0, at * kRowWords, 0u, 0u, 0, (uint32_t)at};
        at += n;
    }
    hipError_t e = hipMemcpyAsync(c->arena + L.jobs, c->h_in, L.in_end - L.jobs, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return fail(c, "hipMemcpyAsync (mapper in)", e);
    Args a;
    a.kmer = reinterpret_cast<const uint32_t *>(c->arena + H.kmer);
    a.gpos = reinterpret_cast<const uint32_t *>(c->arena + H.gpos);
    a.dir = reinterpret_cast<const uint32_t *>(c->arena + H.dir);
    a.toff = reinterpret_cast<const uint32_t *>(c->arena + H.toff);
    a.tlen = reinterpret_cast<const uint32_t *>(c->arena + H.tlen);
    a.nent = (uint32_t)c->set.kmer.size(), a.ntarget = (uint32_t)c->set.len.size();
    a.reads = reinterpret_cast<const Read *>(c->arena + L.reads);
    a.seq = c->arena;
    a.jobs = reinterpret_cast<Job *>(c->arena + L.jobs);
    a.votes = reinterpret_cast<Vote *>(c->arena + L.votes);
    a.nreads = (uint32_t)nr, a.slots = c->slots;
    ccsx_aln::PathArgs b;
    b.jobs = a.jobs, b.seq = c->arena, b.njobs = (uint32_t)nr;
    b.rec = reinterpret_cast<uint32_t *>(c->arena + L.rec);
    b.out = reinterpret_cast<int32_t *>(c->arena + L.out);
    b.words = reinterpret_cast<uint32_t *>(c->arena + L.words);
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(nr, (uint64_t)c->ncu * 8u);
    if ((e = hipEventRecord(c->ev[0], c->stream)) != hipSuccess) return fail(c, "hipEventRecord", e);
    if ((e = ccsx_launch_ref_vote(&a, blocks, c->stream)) != hipSuccess) return fail(c, "vote launch", e);
    if ((e = hipEventRecord(c->ev[1], c->stream)) != hipSuccess) return fail(c, "hipEventRecord", e);
    if ((e = ccsx_launch_band_align_path(&b, blocks, c->stream)) != hipSuccess) return fail(c, "band_align launch", e);
    if ((e = hipEventRecord(c->ev[2], c->stream)) != hipSuccess) return fail(c, "hipEventRecord", e);
    e = hipMemcpyAsync(c->h_out, c->arena + L.votes, L.out_end - L.votes, hipMemcpyDeviceToHost, c->stream);
    if (e != hipSuccess) return fail(c, "hipMemcpyAsync (mapper out)", e);
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return fail(c, "reference mapping", e);
    float ms = 0;
    if (kernel_ms && hipEventElapsedTime(&ms, c->ev[0], c->ev[1]) == hipSuccess) kernel_ms[0] += ms;
    if (kernel_ms && hipEventElapsedTime(&ms, c->ev[1], c->ev[2]) == hipSuccess) kernel_ms[1] += ms;
    const Vote *v = reinterpret_cast<const Vote *>(c->h_out);
    const ccsx_pairaln *pa = reinterpret_cast<const ccsx_pairaln *>(c->h_out + (L.out - L.votes));
    const uint32_t *w = reinterpret_cast<const uint32_t *>(c->h_out + (L.words - L.votes));
    at = 0;
    for (size_t r = 0; r < nr; ++r) {
        const uint32_t n = z[lo + r].len;
        ccsx_ref_rec &rec = recs[lo + r];
        uint32_t *wr = words ? words + woff[lo + r] : nullptr;
        if (v[r].overflow) {
            ++c->stats[4];
            host_read(c, z[lo + r], &rec, wr);
        } else if (v[r].g < 0 || !pa[r].aln) {
            // no vote, or the all-zero band result: unmapped
            memset(&rec, 0, sizeof rec);
            rec.g = -1;
            if (wr)
                for (uint32_t k = 0; k < n; ++k) wr[k] = CCSX_MAP_INS;
        } else {
            rec.g = v[r].g, rec.o = v[r].o, rec.d0 = v[r].d0, rec.votes = v[r].votes, rec.votes2 = v[r].votes2;
            rec.a = pa[r];
            if (wr) memcpy(wr, w + at, (size_t)n * 4);
        }
        at += n;
    }
    ++c->stats[1];
    return true;
}

}  // namespace

extern "C" {

int ccsx_gpu_ref_open(int device, uint64_t max_bytes, ccsx_ref_ctx **out)
{
    *out = nullptr;
    auto *c = new ccsx_ref_ctx();
    c->device = device;
    c->max_bytes = max_bytes ? max_bytes : kDefaultBytes;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    for (int k = 0; k < 3 && e == hipSuccess; ++k) e = hipEventCreate(&c->ev[k]);
    if (e != hipSuccess) {
        fprintf(stderr, "[ccsx_gpu] cannot open a reference mapper on device %d: %s\n", device, hipGetErrorString(e));
        ccsx_gpu_ref_close(c);
        return -1;
    }
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && n > 0) c->ncu = (uint32_t)n;
    *out = c;
    return 0;
}

void ccsx_gpu_ref_close(ccsx_ref_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->arena) (void)hipFree(c->arena);
    if (c->h_in) (void)hipHostFree(c->h_in);
    if (c->h_out) (void)hipHostFree(c->h_out);
    for (hipEvent_t ev : c->ev)
        if (ev) (void)hipEventDestroy(ev);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char *ccsx_gpu_ref_error(const ccsx_ref_ctx *c) { return c ? c->err.c_str() : "no context"; }

int ccsx_gpu_ref_set(ccsx_ref_ctx *c, const ccsx_ref_set *set)
{
    if (!c) return -1;
    std::lock_guard<std::mutex> g(c->mu);
    if (!set || set->len.empty() || set->len.size() > kMaxSet || set->codes.size() > kMaxLetters) {
        c->err = "ccsx_gpu_ref_set: not a reference set (1..64 sequences of at least 13 letters, at most 1,048,576 in all)";
        return -1;
    }
    if (Head(*set).end + Layout(0, 1, 0).end > c->max_bytes) {
        c->err = "ccsx_gpu_ref_set: the set does not fit the arena";
        return -1;
    }
    c->set = *set;
    c->set_on_device = false;
    ++c->stats[2];
    return 0;
}

int ccsx_gpu_ref_vote_cap(ccsx_ref_ctx *c, uint32_t slots)
{
    if (!c) return -1;
    std::lock_guard<std::mutex> g(c->mu);
    if (slots < kMinVoteSlots || slots > kVoteSlots || (slots & (slots - 1u))) {
        c->err = "ccsx_gpu_ref_vote_cap: a power of two in 64 .. 4096";
        return -1;
    }
    c->slots = slots;
    return 0;
}

int ccsx_gpu_ref_map(ccsx_ref_ctx *c, const ccsx_scan_in *z, size_t n, ccsx_ref_rec *recs, uint32_t *words, float *kernel_ms)
{
    if (!c) return -1;
    std::lock_guard<std::mutex> g(c->mu);
    if (kernel_ms) kernel_ms[0] = kernel_ms[1] = 0;
    if (c->set.len.empty()) {
        c->err = "ccsx_gpu_ref_map: no reference set";
        return -1;
    }
    if (n == 0) return 0;
    if (!z || !recs) {
        c->err = "ccsx_gpu_ref_map: null argument";
        return -1;
    }
    for (size_t r = 0; r < n; ++r)
        if (z[r].len && !z[r].ccs) {
            c->err = "ccsx_gpu_ref_map: read " + std::to_string(r) + " has bases but none to read";
            return -1;
        }
    const hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) {
        fail(c, "hipSetDevice", e);
        return -1;
    }
    std::vector<uint64_t> woff(n);
    uint64_t total = 0;
    for (size_t r = 0; r < n; ++r) woff[r] = total, total += z[r].len;
    const uint64_t head = Head(c->set).end;
    size_t lo = 0;
    uint64_t bases = 0;
    auto flush = [&](size_t hi) {
        const bool ok = hi == lo || run_slice(c, z, lo, hi, bases, woff.data(), recs, words, kernel_ms);
        lo = hi, bases = 0;
        return ok;
    };
    for (size_t r = 0; r < n; ++r) {
        const uint64_t len = z[r].len;
        // (a slice's word offsets are 32-bit: its bases stay below 2^32 with any arena)
        if (len >= ccsx_aln::kMaxLen || Layout(head, 1, len).end > c->max_bytes) {
            if (!flush(r)) return -1;
            host_read(c, z[r], &recs[r], words ? words + woff[r] : nullptr);
            lo = r + 1;
            continue;
        }
        if ((Layout(head, r - lo + 1, bases + len).end > c->max_bytes || bases + len > 0xFFFFFFFFull) && !flush(r)) return -1;
        bases += len;
    }
    if (!flush(n)) return -1;
    c->stats[0] += n;
    for (size_t r = 0; r < n; ++r) c->stats[3] += recs[r].g >= 0;
    return 0;
}

int ccsx_gpu_ref_stats(const ccsx_ref_ctx *c, uint64_t *stats, uint32_t n)
{
    if (!c || !stats) return -1;
    for (uint32_t i = 0; i < n && i < 6; ++i) stats[i] = c->stats[i];
    return 0;
}

}  // extern "C"
