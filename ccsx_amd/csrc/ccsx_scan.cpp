// ccsx_scan.cpp -- host side of the adapter scanner (include/ccsx_gpu.h,
// ccsx_gpu_scan_*; the kernel is ccsx_scan.hip).
//
// A scanner context owns one stream, the pattern table of its current set on
// the device (at most 128 patterns, replaced by ccsx_gpu_scan_set), one device
// arena (at most max_bytes, allocated at the first call and grown as slices
// need) and pinned staging, as the demultiplexer's does (ccsx_barcode.cpp).
// ccsx_gpu_scan cuts its reads, in order, into slices that fit the arena; a
// slice is, from the arena's start: what goes in (the reads' codes, one byte
// per base and padded to the kernel's 8-byte words, an offset and a length per
// read, the tile jobs and the zeroed counter) and what comes out (the
// candidate buffer; with tracks, the bottom rows).  Per slice: one copy in, one
// launch, the counter back, then the candidates it counted.
//
// The buffer's first capacity is a guess (one candidate per 32 columns, far
// above an adapter every few hundred bases).  The counter counts every
// candidate, so a slice that overflowed runs once more with the counted
// capacity if that fits max_bytes; else it is halved, and a single read that
// does not fit is scanned by the host's loop (host/scan.cpp) inside the call.
// The call's candidates are then finished on the host (ccsx_scan::finish: fold
// the orientations, the hit rule, the starts, the order).
#include "ccsx_gpu.h"
#include "ccsx_host.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#define CCSX_SCAN_HOST_API
#include "ccsx_scan.h"

extern "C" hipError_t ccsx_launch_scan(const ccsx_scan::Args *a, uint32_t rows, int track, hipStream_t s);

struct ccsx_scan_ctx {
    int device = 0;
    uint64_t max_bytes = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    ccsx_scan::Pat *pats = nullptr;  // device: the current set, npat patterns
    uint32_t npat = 0, rows = 0, T = 0;
    std::string seqs;                // the current set, as given
    std::vector<uint32_t> off, len;
    uint8_t *arena = nullptr;
    uint64_t arena_bytes = 0;
    uint8_t *h_in = nullptr, *h_out = nullptr;  // pinned staging
    uint64_t h_in_bytes = 0, h_out_bytes = 0;
    std::vector<ccsx_scan::HostCand> cands;  // of the call under way
    std::vector<ccsx_scan_hit> hits;         // of the last call
    uint64_t stats[6] = {0, 0, 0, 0, 0, 0};
    std::string err;
    std::mutex mu;
};

namespace {

using namespace ccsx_scan;

constexpr uint64_t kDefaultBytes = 256ull << 20;  // ~16,000 reads of 15 kb per slice
constexpr uint64_t kAlign = 256;
constexpr uint64_t kColsPerCand = 32, kMinCap = 64;

inline uint64_t up(uint64_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

// §1's coding as a table: the host codes every base of every read, once per call
struct CodeTable {
    uint8_t c[256];
    CodeTable()
    {
        for (int ch = 0; ch < 256; ++ch) c[ch] = (uint8_t)ccsx_pol::base_code((uint8_t)ch);
    }
};
const CodeTable kCode;

// what a run of reads sums to
struct Sum {
    uint64_t nr = 0, text = 0, jobs = 0, cols = 0;
    void add(uint32_t n) { ++nr, text += text_bytes(n), jobs += n / kTC + 1, cols += (uint64_t)n + 1; }
    uint64_t cap0() const { return cols / kColsPerCand + kMinCap; }
};

// the offsets of a slice's parts from the arena's start
struct Layout {
    uint64_t text, roff, rlen, jobs, toff, count, in_end, cand, track, end;
    Layout(const Sum &s, uint64_t cap, uint64_t track_bytes)
    {
        text = 0;
        roff = up(s.text);
        rlen = roff + up(s.nr * 4);
        jobs = rlen + up(s.nr * 4);
        toff = jobs + up(s.jobs * sizeof(Job));
        count = toff + (track_bytes ? up(s.nr * 8) : 0);
        in_end = count + kAlign;
        cand = in_end;
        track = cand + up(cap * sizeof(Cand));
        end = track + up(track_bytes);
    }
};

bool fail(ccsx_scan_ctx *c, const char *what, hipError_t e)
{
    c->err = std::string(what) + ": " + hipGetErrorString(e);
    return false;
}

bool grow_pinned(ccsx_scan_ctx *c, uint8_t *&p, uint64_t &have, uint64_t need)
{
    if (need <= have) return true;
    if (p) (void)hipHostFree(p);
    p = nullptr, have = 0;
    need = std::max<uint64_t>(need + need / 4, 1u << 16);
    const hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&p), need, hipHostMallocDefault);
    if (e != hipSuccess) return fail(c, "hipHostMalloc (scanner staging)", e);
    have = need;
    return true;
}

bool grow_arena(ccsx_scan_ctx *c, uint64_t need)
{
    if (need <= c->arena_bytes) return true;
    if (c->arena) (void)hipFree(c->arena);
    c->arena = nullptr, c->arena_bytes = 0;
    // a quarter ahead, never past max_bytes (nor below the need)
    need = std::max(need, std::min<uint64_t>(c->max_bytes, need + need / 4));
    const hipError_t e = hipMalloc(reinterpret_cast<void **>(&c->arena), need);
    if (e != hipSuccess) return fail(c, "hipMalloc (scanner arena)", e);
    c->arena_bytes = need;
    return true;
}

Sum sum_of(const ccsx_scan_in *z, size_t lo, size_t hi)
{
    Sum s;
    for (size_t r = lo; r < hi; ++r) s.add(z[r].len);
    return s;
}

// z[lo .. hi) as one slice with a buffer of cap candidates: stages, launches
// and reads the counter back.  track: the bottom rows go to it as well.
bool launch_slice(ccsx_scan_ctx *c, const ccsx_scan_in *z, size_t lo, size_t hi, const Sum &s, uint64_t cap, int8_t *track,
                  uint64_t track_bytes, uint64_t &count, float *kernel_ms)
{
    const Layout L(s, cap, track_bytes);
    if (!grow_arena(c, L.end) || !grow_pinned(c, c->h_in, c->h_in_bytes, L.in_end) ||
        !grow_pinned(c, c->h_out, c->h_out_bytes, sizeof(uint64_t)))
        return false;
    uint32_t *roff = reinterpret_cast<uint32_t *>(c->h_in + L.roff), *rlen = reinterpret_cast<uint32_t *>(c->h_in + L.rlen);
    Job *jobs = reinterpret_cast<Job *>(c->h_in + L.jobs);
    uint64_t *toff = reinterpret_cast<uint64_t *>(c->h_in + L.toff);
    uint64_t at = 0, nj = 0, tat = 0;
    for (size_t r = lo; r < hi; ++r) {
        const uint32_t n = z[r].len, k = (uint32_t)(r - lo);
        uint8_t *t = c->h_in + L.text + at;
        const uint8_t *q = reinterpret_cast<const uint8_t *>(z[r].ccs);
        for (uint32_t b = 0; b < n; ++b) t[b] = kCode.c[q[b]];
        memset(t + n, 0, text_bytes(n) - n);
        roff[k] = (uint32_t)(at / 8), rlen[k] = n;
        at += text_bytes(n);
        for (uint32_t t0 = 0; t0 <= n; t0 += kTC) jobs[nj++] = Job{k, t0};
        if (track_bytes) toff[k] = tat, tat += (uint64_t)c->npat * ((uint64_t)n + 1);
    }
    memset(c->h_in + L.count, 0, sizeof(uint64_t));
    hipError_t e = hipMemcpyAsync(c->arena, c->h_in, L.in_end, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return fail(c, "hipMemcpyAsync (scanner in)", e);
    Args a;
    a.pats = c->pats;
    a.text = c->arena + L.text;
    a.roff = reinterpret_cast<const uint32_t *>(c->arena + L.roff);
    a.rlen = reinterpret_cast<const uint32_t *>(c->arena + L.rlen);
    a.jobs = reinterpret_cast<const Job *>(c->arena + L.jobs);
    a.count = reinterpret_cast<unsigned long long *>(c->arena + L.count);
    a.cand = reinterpret_cast<Cand *>(c->arena + L.cand);
    a.track = reinterpret_cast<int8_t *>(c->arena + L.track);
    a.toff = reinterpret_cast<const uint64_t *>(c->arena + L.toff);
    a.cap = cap, a.njobs = (uint32_t)nj, a.npat = c->npat;
    if ((e = hipEventRecord(c->ev0, c->stream)) != hipSuccess) return fail(c, "hipEventRecord", e);
    if ((e = ccsx_launch_scan(&a, c->rows, track_bytes != 0, c->stream)) != hipSuccess) return fail(c, "scan launch", e);
    if ((e = hipEventRecord(c->ev1, c->stream)) != hipSuccess) return fail(c, "hipEventRecord", e);
    e = hipMemcpyAsync(c->h_out, c->arena + L.count, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream);
    if (e != hipSuccess) return fail(c, "hipMemcpyAsync (scanner count)", e);
    if (track_bytes && (e = hipMemcpyAsync(track, c->arena + L.track, track_bytes, hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
        return fail(c, "hipMemcpyAsync (scanner tracks)", e);
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return fail(c, "scan", e);
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->ev0, c->ev1) == hipSuccess && kernel_ms) *kernel_ms += ms;
    memcpy(&count, c->h_out, sizeof count);
    ++c->stats[1];
    return true;
}

// the count candidates of the slice z[lo ..) that was just run, appended to the call's
bool fetch(ccsx_scan_ctx *c, size_t lo, const Sum &s, uint64_t cap, uint64_t count)
{
    if (!count) return true;
    const Layout L(s, cap, 0);
    if (!grow_pinned(c, c->h_out, c->h_out_bytes, count * sizeof(Cand))) return false;
    hipError_t e = hipMemcpyAsync(c->h_out, c->arena + L.cand, count * sizeof(Cand), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, "hipMemcpyAsync (scanner candidates)", e);
    const Cand *d = reinterpret_cast<const Cand *>(c->h_out);
    c->cands.reserve(c->cands.size() + count);
    for (uint64_t k = 0; k < count; ++k)
        c->cands.push_back(HostCand{(uint32_t)(lo + (d[k].w0 >> kPatBits)), d[k].w0 & ((1u << kPatBits) - 1u), d[k].w1 & kMaxCol,
                                    (int32_t)(d[k].w1 >> kColBits)});
    c->stats[3] += count;
    return true;
}

// z[lo .. hi): as one slice if it fits, else in halves; one read that does not
// fit goes to the host
bool run_range(ccsx_scan_ctx *c, const ccsx_scan_in *z, size_t lo, size_t hi, float *kernel_ms)
{
    const Sum s = sum_of(z, lo, hi);
    auto split = [&]() {
        if (hi - lo > 1) {
            const size_t mid = lo + (hi - lo) / 2;
            return run_range(c, z, lo, mid, kernel_ms) && run_range(c, z, mid, hi, kernel_ms);
        }
        const size_t before = c->cands.size();
        candidates(c->seqs.data(), c->off.data(), c->len.data(), (uint32_t)c->len.size(), c->T, z[lo].ccs, z[lo].len, (uint32_t)lo,
                   c->cands);
        c->stats[3] += c->cands.size() - before;
        ++c->stats[5];
        return true;
    };
    uint64_t cap = s.cap0();
    if (Layout(s, cap, 0).end > c->max_bytes) {
        // the guess may shrink to what is left, down to one record
        const uint64_t in = Layout(s, 0, 0).end;
        if (in + kAlign > c->max_bytes || s.nr > kMaxReads || s.jobs > 0x7FFFFFFFull) return split();
        cap = (c->max_bytes - in) / kAlign * kAlign / sizeof(Cand);
    }
    uint64_t count = 0;
    if (!launch_slice(c, z, lo, hi, s, cap, nullptr, 0, count, kernel_ms)) return false;
    if (count > cap) {
        if (Layout(s, count, 0).end > c->max_bytes) return split();
        cap = count;
        ++c->stats[4];
        if (!launch_slice(c, z, lo, hi, s, cap, nullptr, 0, count, kernel_ms)) return false;
        if (count > cap) {
            c->err = "ccsx_gpu_scan: the second run counted more candidates than the first";
            return false;
        }
    }
    return fetch(c, lo, s, cap, count);
}

bool ready(ccsx_scan_ctx *c, const char *who, const ccsx_scan_in *z, size_t n)
{
    if (!c->npat) {
        c->err = std::string(who) + ": no adapter set";
        return false;
    }
    if (n && !z) {
        c->err = std::string(who) + ": null argument";
        return false;
    }
    for (size_t r = 0; r < n; ++r)
        if (z[r].len > kMaxCol || (z[r].len && !z[r].ccs)) {
            c->err = std::string(who) + ": read " + std::to_string(r) + " has more than 16,777,215 bases, or none to read";
            return false;
        }
    const hipError_t e = hipSetDevice(c->device);
    return e == hipSuccess || fail(c, "hipSetDevice", e);
}

}  // namespace

extern "C" {

int ccsx_gpu_scan_open(int device, uint64_t max_bytes, ccsx_scan_ctx **out)
{
    *out = nullptr;
    auto *c = new ccsx_scan_ctx();
    c->device = device;
    c->max_bytes = max_bytes ? max_bytes : kDefaultBytes;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&c->ev0);
    if (e == hipSuccess) e = hipEventCreate(&c->ev1);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&c->pats), 2 * kMaxSet * sizeof(Pat));
    if (e != hipSuccess) {
        fprintf(stderr, "[ccsx_gpu] cannot open a scanner on device %d: %s\n", device, hipGetErrorString(e));
        ccsx_gpu_scan_close(c);
        return -1;
    }
    *out = c;
    return 0;
}

void ccsx_gpu_scan_close(ccsx_scan_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->arena) (void)hipFree(c->arena);
    if (c->pats) (void)hipFree(c->pats);
    if (c->h_in) (void)hipHostFree(c->h_in);
    if (c->h_out) (void)hipHostFree(c->h_out);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char *ccsx_gpu_scan_error(const ccsx_scan_ctx *c) { return c ? c->err.c_str() : "no context"; }

int ccsx_gpu_scan_set(ccsx_scan_ctx *c, const char *seqs, const uint32_t *off, const uint32_t *len, uint32_t A, uint32_t T)
{
    if (!c) return -1;
    std::lock_guard<std::mutex> g(c->mu);
    if (ccsx_scan_check(seqs, off, len, A, T) != 0) {
        c->err = "ccsx_gpu_scan_set: not an adapter set (1..64 sequences of 1..64 ACGT letters, threshold 1..100)";
        return -1;
    }
    uint32_t maxlen = 0;
    for (uint32_t a = 0; a < A; ++a) maxlen = std::max(maxlen, len[a]);
    const uint32_t rows = rows_of(maxlen);
    std::vector<Pat> t(2 * (size_t)A);
    for (uint32_t a = 0; a < A; ++a)
        for (uint32_t o = 0; o < 2; ++o) t[2 * a + o] = make_pat(seqs + off[a], len[a], o, rows, T);
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = hipMemcpyAsync(c->pats, t.data(), t.size() * sizeof(Pat), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        c->npat = 0;
        fail(c, "ccsx_gpu_scan_set", e);
        return -1;
    }
    // the set as given, packed: the host finishes the hits with it
    c->seqs.clear(), c->off.clear(), c->len.assign(len, len + A);
    for (uint32_t a = 0; a < A; ++a) c->off.push_back((uint32_t)c->seqs.size()), c->seqs.append(seqs + off[a], len[a]);
    c->npat = 2 * A, c->rows = rows, c->T = T;
    ++c->stats[2];
    return 0;
}

int ccsx_gpu_scan(ccsx_scan_ctx *c, const ccsx_scan_in *z, size_t n, const ccsx_scan_hit **hits, uint64_t *nhits, float *kernel_ms)
{
    if (!c) return -1;
    std::lock_guard<std::mutex> g(c->mu);
    if (kernel_ms) *kernel_ms = 0;
    if (hits) *hits = nullptr;
    if (nhits) *nhits = 0;
    c->hits.clear(), c->cands.clear();
    if (!ready(c, "ccsx_gpu_scan", z, n)) return -1;
    // slices: reads in order while the slice and its first buffer fit
    for (size_t lo = 0; lo < n;) {
        Sum s;
        size_t hi = lo;
        while (hi < n) {
            Sum t = s;
            t.add(z[hi].len);
            if (hi > lo && (Layout(t, t.cap0(), 0).end > c->max_bytes || t.nr > kMaxReads || t.jobs > 0x7FFFFFFFull)) break;
            s = t, ++hi;
        }
        if (!run_range(c, z, lo, hi, kernel_ms)) return -1;
        lo = hi;
    }
    c->stats[0] += n;
    finish(c->cands, c->seqs.data(), c->off.data(), c->len.data(), z, c->hits);
    c->cands.clear();
    if (hits) *hits = c->hits.data();
    if (nhits) *nhits = c->hits.size();
    return 0;
}

int ccsx_gpu_scan_tracks(ccsx_scan_ctx *c, const ccsx_scan_in *z, size_t n, int8_t *track, uint64_t track_bytes)
{
    if (!c) return -1;
    std::lock_guard<std::mutex> g(c->mu);
    if (!ready(c, "ccsx_gpu_scan_tracks", z, n)) return -1;
    const Sum s = sum_of(z, 0, n);
    if (!n) return 0;
    if (!track || track_bytes != (uint64_t)c->npat * s.cols) {
        c->err = "ccsx_gpu_scan_tracks: the track buffer is not 2 A (len + 1) bytes per read";
        return -1;
    }
    if (Layout(s, s.cap0(), track_bytes).end > c->max_bytes || s.nr > kMaxReads || s.jobs > 0x7FFFFFFFull) {
        c->err = "ccsx_gpu_scan_tracks: the reads and their tracks do not fit one slice";
        return -1;
    }
    uint64_t count = 0;
    return launch_slice(c, z, 0, n, s, s.cap0(), track, track_bytes, count, nullptr) ? 0 : -1;
}

int ccsx_gpu_scan_tile(uint32_t rows, uint32_t *TC, uint32_t *WU)
{
    if (rows != 16 && rows != 32 && rows != 48 && rows != 64) return -1;
    if (TC) *TC = kTC;
    if (WU) *WU = warmup_of(rows);
    return 0;
}

int ccsx_gpu_scan_stats(const ccsx_scan_ctx *c, uint64_t *stats, uint32_t n)
{
    if (!c || !stats) return -1;
    for (uint32_t i = 0; i < n && i < 6; ++i) stats[i] = c->stats[i];
    return 0;
}

}  // extern "C"
