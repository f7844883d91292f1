// ccsx_barcode.cpp -- host side of the demultiplexer (include/ccsx_gpu.h,
// ccsx_gpu_bc_*; the kernel is ccsx_barcode.hip).
//
// A demultiplexer context owns one stream, the pattern table of its current
// set on the device (at most 128 KiB, replaced by ccsx_gpu_bc_set), one device
// arena (at most max_bytes, allocated at the first call and grown as slices
// need) and two pinned staging buffers, as the polisher's does
// (ccsx_polish.cpp).  ccsx_gpu_bc_score cuts its ZMWs, in order, into slices
// that fit the arena; a slice is, from the arena's start: what goes in (two
// windows of Wn code bytes and one window length per ZMW) and what comes out
// (40 bytes per ZMW).  Per slice: one copy in, one launch, one copy out.  The
// reads themselves never cross: only their two ends.
#include "ccsx_gpu.h"
#include "ccsx_host.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "ccsx_barcode.h"

extern "C" hipError_t ccsx_launch_barcode(const ccsx_bc::Args *a, uint32_t rows, uint32_t blocks, hipStream_t s);

struct ccsx_bc_ctx {
    int device = 0;
    uint64_t max_bytes = 0;
    uint32_t ncu = 256;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    ccsx_bc::Pat *pats = nullptr;  // device: the current set, nchunks * 64 patterns
    uint32_t nchunks = 0, rows = 0, wn = 0;
    uint8_t *arena = nullptr;
    uint64_t arena_bytes = 0;
    uint8_t *h_in = nullptr, *h_out = nullptr;  // pinned staging
    uint64_t h_in_bytes = 0, h_out_bytes = 0;
    uint64_t stats[3] = {0, 0, 0};
    std::string err;
    std::mutex mu;
};

namespace {

using namespace ccsx_bc;

constexpr uint64_t kDefaultBytes = 64ull << 20;  // ~270,000 ZMWs per slice at Wn = 96
constexpr uint64_t kAlign = 256;
constexpr uint64_t kPatBytes = 2ull * kMaxSet * sizeof(Pat);

inline uint64_t up(uint64_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

// the offsets of a slice's parts from the arena's start
struct Layout {
    uint64_t win, wlen, in_end, out, end;
    Layout(uint64_t nz, uint32_t wn)
    {
        win = 0;
        wlen = up(nz * 2 * wn);
        in_end = wlen + up(nz * 4);
        out = in_end;
        end = out + up(nz * sizeof(ccsx_bc_out));
    }
};

bool fail(ccsx_bc_ctx *c, const char *what, hipError_t e)
{
    c->err = std::string(what) + ": " + hipGetErrorString(e);
    return false;
}

bool grow_pinned(ccsx_bc_ctx *c, uint8_t *&p, uint64_t &have, uint64_t need)
{
    if (need <= have) return true;
    if (p) (void)hipHostFree(p);
    p = nullptr, have = 0;
    need = std::max<uint64_t>(need + need / 4, 1u << 16);
    const hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&p), need, hipHostMallocDefault);
    if (e != hipSuccess) return fail(c, "hipHostMalloc (demultiplexer staging)", e);
    have = need;
    return true;
}

bool grow_arena(ccsx_bc_ctx *c, uint64_t need)
{
    if (need <= c->arena_bytes) return true;
    if (c->arena) (void)hipFree(c->arena);
    c->arena = nullptr, c->arena_bytes = 0;
    // a quarter ahead, never past max_bytes (nor below the need)
    need = std::max(need, std::min<uint64_t>(c->max_bytes, need + need / 4));
    const hipError_t e = hipMalloc(reinterpret_cast<void **>(&c->arena), need);
    if (e != hipSuccess) return fail(c, "hipMalloc (demultiplexer arena)", e);
    c->arena_bytes = need;
    return true;
}

// z[0 .. n) as one slice
bool run_slice(ccsx_bc_ctx *c, const ccsx_bc_in *z, size_t n, ccsx_bc_out *out, float *kernel_ms)
{
    const uint32_t wn = c->wn;
    const Layout L(n, wn);
    if (!grow_arena(c, L.end) || !grow_pinned(c, c->h_in, c->h_in_bytes, L.in_end) ||
        !grow_pinned(c, c->h_out, c->h_out_bytes, L.end - L.out))
        return false;
    uint32_t *wl = reinterpret_cast<uint32_t *>(c->h_in + L.wlen);
    for (size_t s = 0; s < n; ++s) {
        const uint32_t len = z[s].len, w = std::min(len, wn);
        uint8_t *e0 = c->h_in + L.win + (2 * s) * wn, *e1 = e0 + wn;
        const uint8_t *q = reinterpret_cast<const uint8_t *>(z[s].ccs);
        for (uint32_t k = 0; k < w; ++k) {
            e0[k] = (uint8_t)ccsx_pol::base_code(q[k]);
            e1[k] = (uint8_t)(3u - ccsx_pol::base_code(q[len - 1 - k]));
        }
        memset(e0 + w, 0, wn - w), memset(e1 + w, 0, wn - w);
        wl[s] = w;
    }
    hipError_t e = hipMemcpyAsync(c->arena, c->h_in, L.in_end, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return fail(c, "hipMemcpyAsync (demultiplexer in)", e);
    Args a;
    a.pats = c->pats;
    a.win = c->arena + L.win;
    a.wlen = reinterpret_cast<const uint32_t *>(c->arena + L.wlen);
    a.out = reinterpret_cast<int32_t *>(c->arena + L.out);
    a.njobs = (uint32_t)(2 * n), a.nchunks = c->nchunks, a.wn = wn;
    // one-wave workgroups: 32 of them fill a CU's wave slots
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(2 * n, (uint64_t)c->ncu * 32u);
    if ((e = hipEventRecord(c->ev0, c->stream)) != hipSuccess) return fail(c, "hipEventRecord", e);
    if ((e = ccsx_launch_barcode(&a, c->rows, blocks, c->stream)) != hipSuccess) return fail(c, "barcode launch", e);
    if ((e = hipEventRecord(c->ev1, c->stream)) != hipSuccess) return fail(c, "hipEventRecord", e);
    e = hipMemcpyAsync(c->h_out, c->arena + L.out, n * sizeof(ccsx_bc_out), hipMemcpyDeviceToHost, c->stream);
    if (e != hipSuccess) return fail(c, "hipMemcpyAsync (demultiplexer out)", e);
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return fail(c, "barcode score", e);
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->ev0, c->ev1) == hipSuccess && kernel_ms) *kernel_ms += ms;
    memcpy(out, c->h_out, n * sizeof(ccsx_bc_out));
    ++c->stats[1];
    return true;
}

}  // namespace

static_assert(sizeof(ccsx_bc_out) == 40, "five words per end");

extern "C" {

int ccsx_gpu_bc_open(int device, uint64_t max_bytes, ccsx_bc_ctx **out)
{
    *out = nullptr;
    auto *c = new ccsx_bc_ctx();
    c->device = device;
    // (at least one ZMW of the widest window fits)
    c->max_bytes = std::max<uint64_t>(max_bytes ? max_bytes : kDefaultBytes, Layout(1, kMaxWin).end);
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&c->ev0);
    if (e == hipSuccess) e = hipEventCreate(&c->ev1);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&c->pats), kPatBytes);
    if (e != hipSuccess) {
        fprintf(stderr, "[ccsx_gpu] cannot open a demultiplexer on device %d: %s\n", device, hipGetErrorString(e));
        ccsx_gpu_bc_close(c);
        return -1;
    }
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && n > 0) c->ncu = (uint32_t)n;
    *out = c;
    return 0;
}

void ccsx_gpu_bc_close(ccsx_bc_ctx *c)
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

const char *ccsx_gpu_bc_error(const ccsx_bc_ctx *c) { return c ? c->err.c_str() : "no context"; }

int ccsx_gpu_bc_set(ccsx_bc_ctx *c, const char *seqs, const uint32_t *off, const uint32_t *len, uint32_t B, uint32_t Wn)
{
    if (!c) return -1;
    std::lock_guard<std::mutex> g(c->mu);
    if (Wn < 1 || Wn > kMaxWin || ccsx_barcode_check(seqs, off, len, B) != 0) {
        c->err = "ccsx_gpu_bc_set: not a barcode set (1..2048 sequences of 1..64 ACGT letters, window 1..256)";
        return -1;
    }
    uint32_t maxlen = 0;
    for (uint32_t b = 0; b < B; ++b) maxlen = std::max(maxlen, len[b]);
    const uint32_t rows = rows_of(maxlen), nchunks = (2 * B + kLanes - 1) / kLanes;
    // (the table is staged in pageable memory: once per set, at most 128 KiB)
    std::vector<Pat> t((size_t)nchunks * kLanes, Pat{0, 0, 0, 0, 0});
    for (uint32_t b = 0; b < B; ++b)
        for (uint32_t o = 0; o < 2; ++o) t[2 * b + o] = make_pat(seqs + off[b], len[b], o, rows);
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = hipMemcpyAsync(c->pats, t.data(), t.size() * sizeof(Pat), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        c->nchunks = 0;
        fail(c, "ccsx_gpu_bc_set", e);
        return -1;
    }
    c->nchunks = nchunks, c->rows = rows, c->wn = Wn;
    ++c->stats[2];
    return 0;
}

int ccsx_gpu_bc_score(ccsx_bc_ctx *c, const ccsx_bc_in *z, size_t nz, ccsx_bc_out *out, float *kernel_ms)
{
    if (!c) return -1;
    std::lock_guard<std::mutex> g(c->mu);
    if (kernel_ms) *kernel_ms = 0;
    if (!c->nchunks) {
        c->err = "ccsx_gpu_bc_score: no barcode set";
        return -1;
    }
    if (nz == 0) return 0;
    if (!z || !out) {
        c->err = "ccsx_gpu_bc_score: null argument";
        return -1;
    }
    const hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) {
        fail(c, "hipSetDevice", e);
        return -1;
    }
    // every ZMW costs the same, and the three parts round up by less than
    // kAlign each: ZMWs per slice (one always fits; at most 2^30 jobs per launch)
    const uint64_t each = 2ull * c->wn + 4 + sizeof(ccsx_bc_out);
    const uint64_t per = std::min<uint64_t>(std::max<uint64_t>((c->max_bytes - 3 * kAlign) / each, 1), 1u << 29);
    for (size_t i = 0; i < nz; i += per) {
        const size_t n = std::min<size_t>(per, nz - i);
        if (!run_slice(c, z + i, n, out + i, kernel_ms)) return -1;
        c->stats[0] += n;
    }
    return 0;
}

int ccsx_gpu_bc_stats(const ccsx_bc_ctx *c, uint64_t *stats, uint32_t n)
{
    if (!c || !stats) return -1;
    for (uint32_t i = 0; i < n && i < 3; ++i) stats[i] = c->stats[i];
    return 0;
}

}  // extern "C"
