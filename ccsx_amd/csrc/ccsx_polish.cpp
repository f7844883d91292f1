// ccsx_polish.cpp -- host side of the polisher (include/ccsx_gpu.h,
// ccsx_gpu_polish_*; the kernels are ccsx_polish.hip).
//
// A polisher context owns one stream, one device arena (at most max_bytes,
// allocated at the first call and grown as slices need) and two pinned staging
// buffers, as the aligner's does (ccsx_align.cpp).  ccsx_gpu_polish cuts its
// ZMWs, in order, into slices that fit the arena; a slice is, from the arena's
// start: what goes in (the ZMW table, the job table, the drafts, the segments'
// bytes, their map words), what stays (16 bytes of records, the piece end and
// the piece's last offset per row; 44 bytes of counters per draft position)
// and what comes out (four words per ZMW, the realigned map, the polished
// bases and qualities).  Per slice: one copy in, two memsets, three launches,
// one copy out.  A ZMW with a bad map is answered here; one that no arena of
// max_bytes holds, or beyond the kernels' range, runs ccsx_polish_host here.
#include "ccsx_gpu.h"
#include "ccsx_host.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "ccsx_polish.h"

extern "C" hipError_t ccsx_launch_polish(const ccsx_pol::Args *a, uint32_t job_blocks, uint32_t zmw_blocks, hipStream_t s);

struct ccsx_polish_ctx {
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
    // the last call's results (ccsx_polish_out points into them)
    std::vector<char> r_seq;
    std::vector<uint8_t> r_qual;
    std::vector<uint32_t> r_map;
    std::string err;
    std::mutex mu;
};

namespace {

using namespace ccsx_pol;

constexpr uint64_t kDefaultBytes = 4ull << 30;
constexpr uint64_t kAlign = 256;

inline uint64_t up(uint64_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

// what a slice sums over its ZMWs
struct Sum {
    uint64_t nz = 0, jobs = 0, rows = 0, ccs = 0, cnt = 0, out = 0;  // cnt in words, out in bytes per plane
    void add(uint64_t n, uint64_t j, uint64_t r) { ++nz, jobs += j, rows += r, ccs += n, cnt += (n + 1) * kCounters, out += 2 * n + 1; }
};

// the offsets of a slice's parts from the arena's start
struct Layout {
    uint64_t zmws, jobs, ccs, seq, map, in_end, rec, pend, pl, cnt, hdr, wout, oseq, oqual, end;
    explicit Layout(const Sum &s)
    {
        zmws = 0;
        jobs = up(s.nz * sizeof(Zmw));
        ccs = jobs + up(s.jobs * sizeof(Job));
        seq = ccs + up(s.ccs);
        map = seq + up(s.rows);
        in_end = map + up(s.rows * 4);
        rec = in_end;
        pend = rec + up(s.rows * 16);
        pl = pend + up(s.rows);
        cnt = pl + up(s.rows * 4);
        hdr = cnt + up(s.cnt * 4);
        wout = hdr + up(s.nz * 16);
        oseq = wout + up(s.rows * 4);
        oqual = oseq + up(s.out);
        end = oqual + up(s.out);
    }
};

struct Shape {
    uint64_t rows = 0, jobs = 0;  // the ZMW's bases and its non-empty segments
    uint64_t row0 = 0, out0 = 0;  // its place in the context's result buffers
};

bool fail(ccsx_polish_ctx *c, const char *what, hipError_t e)
{
    c->err = std::string(what) + ": " + hipGetErrorString(e);
    return false;
}

bool grow_pinned(ccsx_polish_ctx *c, uint8_t *&p, uint64_t &have, uint64_t need)
{
    if (need <= have) return true;
    if (p) (void)hipHostFree(p);
    p = nullptr, have = 0;
    need = std::max<uint64_t>(need + need / 4, 1u << 20);
    const hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&p), need, hipHostMallocDefault);
    if (e != hipSuccess) return fail(c, "hipHostMalloc (polisher staging)", e);
    have = need;
    return true;
}

bool grow_arena(ccsx_polish_ctx *c, uint64_t need)
{
    if (need <= c->arena_bytes) return true;
    if (c->arena) (void)hipFree(c->arena);
    c->arena = nullptr, c->arena_bytes = 0;
    // in steps of 64 MiB, a quarter ahead, never past max_bytes (nor below the need)
    const uint64_t step = 64ull << 20;
    need = std::max(need, std::min<uint64_t>(c->max_bytes, (need + need / 4 + step - 1) / step * step));
    const hipError_t e = hipMalloc(reinterpret_cast<void **>(&c->arena), need);
    if (e != hipSuccess) return fail(c, "hipMalloc (polisher arena)", e);
    c->arena_bytes = need;
    return true;
}

// z[idx[0 .. n)] as one slice
bool run_slice(ccsx_polish_ctx *c, const ccsx_polish_in *z, const std::vector<Shape> &shape, const size_t *idx, size_t n,
               const Sum &sum, ccsx_polish_out *out, float *kernel_ms)
{
    const Layout L(sum);
    const uint64_t out_bytes = L.end - L.hdr;
    if (!grow_arena(c, L.end) || !grow_pinned(c, c->h_in, c->h_in_bytes, L.in_end) ||
        !grow_pinned(c, c->h_out, c->h_out_bytes, out_bytes))
        return false;
    Zmw *zt = reinterpret_cast<Zmw *>(c->h_in + L.zmws);
    Job *jt = reinterpret_cast<Job *>(c->h_in + L.jobs);
    uint64_t row = 0, ccs = 0, cnt = 0, ob = 0, nj = 0;
    for (size_t s = 0; s < n; ++s) {
        const ccsx_polish_in &q = z[idx[s]];
        zt[s] = Zmw{ccs, cnt, ob, q.len, 0u};
        memcpy(c->h_in + L.ccs + ccs, q.ccs, q.len);
        uint64_t mo = 0;  // the segment's first word in the ZMW's map
        for (uint32_t k = 0; k < q.nseg; mo += q.seg_len[k], ++k) {
            const uint32_t m = q.seg_len[k];
            if (!m) continue;
            jt[nj++] = Job{row, m, (uint32_t)s};
            memcpy(c->h_in + L.seq + row, q.seqs + q.seg_off[k], m);
            memcpy(c->h_in + L.map + row * 4, q.map + mo, (size_t)m * 4);
            row += m;
        }
        ccs += q.len, cnt += ((uint64_t)q.len + 1) * kCounters, ob += 2 * (uint64_t)q.len + 1;
    }
    hipError_t e = hipMemcpyAsync(c->arena, c->h_in, L.in_end, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return fail(c, "hipMemcpyAsync (polisher in)", e);
    // the counters and the ZMWs' result words are adjacent
    if ((e = hipMemsetAsync(c->arena + L.cnt, 0, L.wout - L.cnt, c->stream)) != hipSuccess)
        return fail(c, "hipMemsetAsync (polisher counters)", e);
    Args a;
    a.zmws = reinterpret_cast<const Zmw *>(c->arena + L.zmws);
    a.jobs = reinterpret_cast<const Job *>(c->arena + L.jobs);
    a.ccs = c->arena + L.ccs;
    a.seq = c->arena + L.seq;
    a.map = reinterpret_cast<const uint32_t *>(c->arena + L.map);
    a.rec = reinterpret_cast<uint64_t *>(c->arena + L.rec);
    a.pend = c->arena + L.pend;
    a.pl = reinterpret_cast<uint32_t *>(c->arena + L.pl);
    a.cnt = reinterpret_cast<uint32_t *>(c->arena + L.cnt);
    a.hdr = reinterpret_cast<uint32_t *>(c->arena + L.hdr);
    a.wout = reinterpret_cast<uint32_t *>(c->arena + L.wout);
    a.oseq = c->arena + L.oseq;
    a.oqual = c->arena + L.oqual;
    a.nzmw = (uint32_t)n, a.njobs = (uint32_t)nj;
    // one-wave workgroups of 28 VGPRs: 32 of them fill a CU's wave slots
    const uint32_t jb = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(nj, 1), (uint64_t)c->ncu * 32u);
    const uint32_t zb = (uint32_t)std::min<uint64_t>(n, (uint64_t)c->ncu * 4u);
    if ((e = hipEventRecord(c->ev0, c->stream)) != hipSuccess) return fail(c, "hipEventRecord", e);
    if ((e = ccsx_launch_polish(&a, jb, zb, c->stream)) != hipSuccess) return fail(c, "polish launch", e);
    if ((e = hipEventRecord(c->ev1, c->stream)) != hipSuccess) return fail(c, "hipEventRecord", e);
    e = hipMemcpyAsync(c->h_out, c->arena + L.hdr, out_bytes, hipMemcpyDeviceToHost, c->stream);
    if (e != hipSuccess) return fail(c, "hipMemcpyAsync (polisher out)", e);
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return fail(c, "polish", e);
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->ev0, c->ev1) == hipSuccess && kernel_ms) *kernel_ms += ms;
    const uint8_t *h = c->h_out;
    row = ob = 0;
    for (size_t s = 0; s < n; ++s) {
        const size_t i = idx[s];
        const Shape &sh = shape[i];
        const uint32_t *hdr = reinterpret_cast<const uint32_t *>(h) + 4 * s;
        const uint64_t cap = 2 * (uint64_t)z[i].len + 1;
        if (hdr[0] > cap) {
            c->err = "polish: a polished read longer than its bound";
            return false;
        }
        memcpy(c->r_map.data() + sh.row0, h + (L.wout - L.hdr) + row * 4, sh.rows * 4);
        memcpy(c->r_seq.data() + sh.out0, h + (L.oseq - L.hdr) + ob, hdr[0]);
        memcpy(c->r_qual.data() + sh.out0, h + (L.oqual - L.hdr) + ob, hdr[0]);
        out[i].len = hdr[0], out[i].nsub = hdr[1], out[i].nins = hdr[2], out[i].ndel = hdr[3];
        row += sh.rows, ob += cap;
    }
    ++c->stats[2];
    return true;
}

}  // namespace

extern "C" {

int ccsx_gpu_polish_open(int device, uint64_t max_bytes, ccsx_polish_ctx **out)
{
    *out = nullptr;
    auto *c = new ccsx_polish_ctx();
    c->device = device;
    c->max_bytes = max_bytes ? max_bytes : kDefaultBytes;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&c->ev0);
    if (e == hipSuccess) e = hipEventCreate(&c->ev1);
    if (e != hipSuccess) {
        fprintf(stderr, "[ccsx_gpu] cannot open a polisher on device %d: %s\n", device, hipGetErrorString(e));
        ccsx_gpu_polish_close(c);
        return -1;
    }
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && n > 0) c->ncu = (uint32_t)n;
    *out = c;
    return 0;
}

void ccsx_gpu_polish_close(ccsx_polish_ctx *c)
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

const char *ccsx_gpu_polish_error(const ccsx_polish_ctx *c) { return c ? c->err.c_str() : "no context"; }

int ccsx_gpu_polish(ccsx_polish_ctx *c, const ccsx_polish_in *z, size_t nz, ccsx_polish_out *out, float *kernel_ms)
{
    if (!c) return -1;
    std::lock_guard<std::mutex> g(c->mu);
    if (kernel_ms) *kernel_ms = 0;
    if (nz == 0) return 0;
    if (!z || !out) {
        c->err = "ccsx_gpu_polish: null argument";
        return -1;
    }
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) {
        fail(c, "hipSetDevice", e);
        return -1;
    }
    // the result buffers, sized before any pointer into them is handed out
    std::vector<Shape> shape(nz);
    uint64_t rows = 0, outb = 0;
    for (size_t i = 0; i < nz; ++i) {
        Shape &s = shape[i];
        for (uint32_t k = 0; k < z[i].nseg; ++k) s.rows += z[i].seg_len[k], s.jobs += z[i].seg_len[k] != 0;
        s.row0 = rows, s.out0 = outb;
        rows += s.rows, outb += 2 * (uint64_t)z[i].len + 1;
    }
    c->r_seq.assign(outb, 0), c->r_qual.assign(outb, 0), c->r_map.assign(std::max<uint64_t>(rows, 1), 0);
    std::vector<size_t> idx;
    Sum sum;
    auto flush = [&]() {
        const bool ok = idx.empty() || run_slice(c, z, shape, idx.data(), idx.size(), sum, out, kernel_ms);
        idx.clear(), sum = Sum();
        return ok;
    };
    for (size_t i = 0; i < nz; ++i) {
        const ccsx_polish_in &q = z[i];
        const Shape &s = shape[i];
        ++c->stats[0], c->stats[1] += q.nseg;
        out[i] = ccsx_polish_out{c->r_seq.data() + s.out0, c->r_qual.data() + s.out0, 0, 0, 0, 0, c->r_map.data() + s.row0, 0};
        if (!map_ok(q.map, q.seg_len, q.nseg, q.len)) {
            out[i].seq = nullptr, out[i].qual = nullptr, out[i].map = nullptr, out[i].status = CCSX_POLISH_BAD_MAP;
            ++c->stats[4];
            continue;
        }
        bool far = q.len >= kMaxLen;
        for (uint32_t k = 0; k < q.nseg; ++k) far |= q.seg_len[k] >= kMaxLen;
        Sum one;
        one.add(q.len, s.jobs, s.rows);
        const bool alone = far || Layout(one).end > c->max_bytes;
        if (alone || q.len == 0) {
            // (an empty draft needs no kernel: nothing to align to)
            uint32_t counts[4];
            ccsx_polish_host(q.ccs, q.len, q.seqs, q.seg_off, q.seg_len, q.nseg, q.map, c->r_seq.data() + s.out0,
                             c->r_qual.data() + s.out0, c->r_map.data() + s.row0, counts);
            out[i].len = counts[0], out[i].nsub = counts[1], out[i].nins = counts[2], out[i].ndel = counts[3];
            c->stats[3] += alone;
            continue;
        }
        Sum with = sum;
        with.add(q.len, s.jobs, s.rows);
        if (Layout(with).end > c->max_bytes) {
            if (!flush()) return -1;
            with = one;
        }
        idx.push_back(i);
        sum = with;
    }
    return flush() ? 0 : -1;
}

int ccsx_gpu_polish_stats(const ccsx_polish_ctx *c, uint64_t *stats, uint32_t n)
{
    if (!c || !stats) return -1;
    for (uint32_t i = 0; i < n && i < 5; ++i) stats[i] = c->stats[i];
    return 0;
}

}  // extern "C"
