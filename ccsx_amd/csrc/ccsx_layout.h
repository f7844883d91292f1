// ccsx_layout.h -- per-ZMW HBM workspace layout, shared by the host launcher
// (sizing, offsets) and the device code (addressing).  See DESIGN.md §3.
//
// One ZMW owns one contiguous workspace slab.  Every capacity is derived from
// S = sum of the ZMW's segment lengths (an upper bound on the rows and edges of
// any POA the ZMW can build, SPEC.md §5) and n = number of segments.
#pragma once
#include <stdint.h>

#ifndef CCSX_HD
#if defined(__HIPCC__)
#define CCSX_HD __host__ __device__
#else
#define CCSX_HD
#endif
#endif

namespace ccsx {

constexpr int kW = 128;        // DP band (main.c:849 bandwidth = 128)
constexpr uint32_t kRecRow = kW;  // bytes of a DP row's cell records (8 bits per cell)
// DP rows back whose H / D a row reads from the LDS ring (farther
// predecessors: HBM spill records); per kernel configuration
#ifndef CCSX_RING
#define CCSX_RING 16
#endif
constexpr int kRing = CCSX_RING;
constexpr int kRowW = 272;     // LDS words per ring row of the two-wave DP: H and D, each [4 pad | 128 | 4 pad]
#ifndef CCSX_RINGA
#define CCSX_RINGA 32
#endif
// its ring rows: kRing predecessor rows + 2 blocks of the helpers' lag (a
// power of two: slot = row & 31; with 8-row blocks, measured 55.05 ms vs
// 57.0 for 24 rows and 4-row blocks, tools/gpu_ab.sh r02o)
constexpr int kRingA = CCSX_RINGA;
constexpr int kNeg = -(1 << 29);
// the HBM-read kernel instance's LDS window of the read: two chunks of
// kWinChunk bases as 2-bit codes (ccsx_kernel.hip win_load)
constexpr uint32_t kWinChunk = 8192;
constexpr uint32_t kRdWinBytes = kWinChunk / 2;
constexpr uint32_t kNone = 0xFFFFFFFFu;
// band offset bits of a row meta word (ZLayout::rmeta)
constexpr uint32_t kMetaOff = 0x3FFFFFu;

// The kernel configurations (ccsx_kernel.hip is compiled once per
// configuration, ccsx_gpu.cpp picks one per slice):
//  * latency: three waves, 8-row lockstep blocks and a 32-row ring -- the
//    shortest per-ZMW chain, 4 workgroups per CU (config B: 1,000 ZMWs in one
//    wave of workgroups);
//  * occupancy: three waves, 4-row blocks and a 24-row ring -- 5 workgroups
//    per CU, for slices larger than the latency configuration keeps resident;
//  * throughput: two waves (one helper), 4-row blocks, a 16-row ring of which
//    the last 8 rows are read back -- up to 8 workgroups per CU, for slices of
//    thousands of ZMWs, where resident ZMWs rather than per-ZMW latency bound
//    the launch;
//  * solo: one wave that also computes the decision bits, an 8-row ring and
//    one traceback buffer -- up to 16 workgroups per CU (~10 KB of LDS each);
//  * solo16: the solo one with an int16 ring (exact for reads of at most
//    16,256 bases), 16-row traceback blocks and 96 VGPRs -- up to 20
//    workgroups per CU (~5.5 KB of LDS each); slices whose pushed reads
//    exceed that, or whose reads live in HBM, run the solo one.
// Each configuration's object reports its own LDS words and threads
// (KCfgInfo), so the host never restates the build flags.
enum KernelCfg : int32_t { kCfgLatency = 0, kCfgOccupancy = 1, kCfgThroughput = 2, kCfgSolo = 3, kCfgSolo16 = 4,
                           kCfgSolo16W = 5, kCfgCount = 6 };
struct KCfgInfo {
    uint32_t lds_fixed_words;  // LDS words before the read buffer
    uint32_t threads;          // workgroup size
    uint32_t ring_rows, ring_back;
    uint32_t waves_per_simd;   // the object's register budget (amdgpu_waves_per_eu)
    uint32_t max_read;         // longest pushed read the object takes on the LDS instance (0: any)
    uint32_t profiling;        // 1: the object carries the per-ZMW phase counters (diagnostic builds)
};

// per-ZMW status codes (0 = ok); any non-zero status is fatal for the batch
enum Status : int32_t {
    kOk = 0,
    kErrRows = 1,      // graph rows exceed rcap
    kErrEdges = 2,     // edges exceed ecap
    kErrMulti = 3,     // (unused: kept so status values stay stable)
    kErrSpill = 4,     // spilled DP rows exceed scap
    kErrInDegree = 5,  // (unused since wide slot records: kept so status values stay stable)
    kErrReadLen = 6,   // pushed read longer than the LDS read buffer (re-run with an uncapped buffer)
    kErrOut = 7,       // CCS longer than the output slab
    kErrTrace = 8,     // traceback did not terminate (internal error)
    kErrBpLog = 9,     // more shredding rounds than the breakpoint log holds (re-run with full caps)
};

enum Mode : int32_t { kShred = 0, kPrimitive = 1, kSinglePoa = 2 };

struct ZmwDesc {
    uint64_t seq_off;   // byte offset of the ZMW's sequence bytes in the seq arena
    uint64_t ws_off;    // byte offset of the workspace slab (256-B aligned)
    uint64_t out_off;   // byte offset of the CCS / consensus output slab
    uint64_t msa_off;   // byte offset of the MSA output slab (kSinglePoa only)
    uint32_t seg0;      // index of the first segment in the segment arrays
    uint32_t n;         // number of segments (pushed reads)
    uint32_t rcap, ecap, lcap, scap, nw;
    uint32_t wcap;      // far-row slot records (rows flagged far: u16 M / D slots per cell)
    uint32_t outcap;    // output slab capacity (bytes)
    uint32_t msacap;    // MSA slab capacity (bytes)
    uint64_t bp_off;    // breakpoint log (-v >= 3): word offset of {rounds, (i, ncols) x bpcap}
    uint32_t bpcap;     // rounds the log holds (0: no log)
    uint32_t pad_;
};

struct ZLayout {
    uint64_t nb0, mem0, poff0, pred0, nb1, mem1, poff1, pred1;
    uint64_t rmeta, spf, sslot, codes, dsl, spill, rrec;
    uint64_t ev, tgt, ipt, iinf, ifix, cnt, fixf, addp, cntn;
    uint64_t colof, cons, cmask, colrow, rdoff, rdlen, rfirst, rlast, rfc, rlc;
    uint64_t ext;  // rarely used regions (zext): kept as one offset to spare registers
    uint64_t total;
};

CCSX_HD inline uint64_t align256(uint64_t x) { return (x + 255) & ~uint64_t(255); }

// Per-base consensus quality (SPEC.md §9): a column whose consensus base is
// carried by `match` of the `cov` reads spanning it scores kQStep per net vote
// (agreeing reads minus spanning reads that disagree or have a gap), clamped
// to [kQMin, kQMax].  Integer only: the device and the host compute the same byte.
constexpr int32_t kQStep = 3, kQMin = 2, kQMax = 93;
CCSX_HD inline uint8_t qual_phred(uint32_t match, uint32_t cov)
{
    const int64_t q = int64_t(kQStep) * (2 * int64_t(match) - int64_t(cov));
    return uint8_t(q < kQMin ? kQMin : q > kQMax ? kQMax : q);
}

// Per-pass alignment statistics (SPEC.md §10): one record per pushed segment,
// the words of ccsx_pass_stat (ccsx_gpu.h) in its order
enum PassWord : uint32_t { kPsMatch = 0, kPsMismatch, kPsIns, kPsDel, kPsCbeg, kPsCend, kPassWords };

// Subread-to-CCS coordinate map (SPEC.md §11): one word per pushed base, the
// CCS offset in bits 0..29 (kBmOffMask) and the two flags
constexpr uint32_t kBmOffMask = (1u << 30) - 1u, kBmMismatch = 1u << 30, kBmIns = 1u << 31;

// Per-base strand pileup (SPEC.md §12): twelve bytes per CCS base, the layout
// of ccsx_pileup (ccsx_gpu.h): per strand (forward reads first) the reads with
// A, C, G, T in the base's column, the spanning reads without a base there, and
// the bases of the dropped (gap-consensus) columns before it.  Every field
// saturates at 255: the device and the host clamp with the same function.
constexpr uint32_t kPuBytes = 12, kPuGap = 4, kPuIns = 5, kPuFields = 6;
CCSX_HD inline uint8_t sat8(uint32_t v) { return uint8_t(v > 255u ? 255u : v); }

// Per-base consensus kinetics (SPEC.md §13): eight bytes per CCS base, the
// layout of ccsx_kinetics (ccsx_gpu.h): per strand (forward reads first) the
// codes of the mean inter-pulse duration and the mean pulse width over the
// reads that carry the consensus base, and their number saturating at 255.
// The 8-bit codec: byte b stands for ((b & 63) << g) + (64 << g) - 64 frames,
// g = b >> 6; kin_code gives the byte nearest to min(f, kKnMaxFrames), the
// lower one on a tie.  Integer only: the device and the host share both.
constexpr uint32_t kKnBytes = 8, kKnMaxFrames = 952;
// words of a column's partial sums while its reads span several mask words
// (per strand: ipd frames, pw frames, reads)
constexpr uint32_t kKnPart = 6;
// a kinetics strand byte (KArgs::ksrev): bit 0 the segment is reverse, bit 1
// its ZMW came without kinetics planes (its records are all zero)
constexpr uint8_t kKnRev = 1, kKnNone = 2;
CCSX_HD inline uint32_t kin_frames(uint32_t b)
{
    const uint32_t g = (b >> 6) & 3u;
    return ((b & 63u) << g) + (64u << g) - 64u;
}
CCSX_HD inline uint8_t kin_code(uint32_t f)
{
    if (f > kKnMaxFrames) f = kKnMaxFrames;
    const uint32_t g = f < 64u ? 0u : f < 192u ? 1u : f < 448u ? 2u : 3u;
    const uint32_t q = f - ((64u << g) - 64u);
    // round to the nearest step, a half down; step 64 of a group is code 0 of the next
    return uint8_t(g * 64u + ((q + (g ? (1u << (g - 1u)) - 1u : 0u)) >> g));
}

// The extension regions, in order (offsets relative to ZLayout::ext):
//  * the far rows' slot records (rows with more than four predecessors or one
//    beyond the DP ring, whose 8-bit cell records carry no tags): per cell the
//    M and D predecessor slots, u16 each, 512 B per far row, taken in the
//    order the DP meets them (the row's index in its tag-plane row, word 0);
//  * the HBM-read kernel instance (reads beyond the LDS read buffer): the read
//    as 2-bit codes and the shredding cursors.
enum ZExt { kExtWtag = 0, kExtRdbuf, kExtPos, kExtEnd };

CCSX_HD inline uint64_t zext_size(const ZmwDesc &d, int which)
{
    switch (which) {
    case kExtWtag: return uint64_t(d.wcap) * kW * 4;
    case kExtRdbuf: return uint64_t((d.lcap + 15) / 16 + 2) * 4;
    default: return uint64_t(d.n) * 4;
    }
}

// offset of extension region `which` from ZLayout::ext (= bytes of the ones before it)
CCSX_HD inline uint64_t zext_bytes(const ZmwDesc &d, int which)
{
    uint64_t o = 0;
    for (int i = 0; i < which; ++i) o = align256(o + zext_size(d, i));
    return o;
}

CCSX_HD inline void zlayout(ZLayout &L, const ZmwDesc &d)
{
    uint64_t o = 0;
    auto take = [&o](uint64_t bytes) {
        uint64_t r = o;
        o = align256(o + bytes);
        return r;
    };
    L.nb0 = take(d.rcap);
    L.mem0 = take(uint64_t(d.rcap) * d.nw * 8);
    L.poff0 = take(uint64_t(d.rcap + 1) * 4);
    L.pred0 = take(uint64_t(d.ecap) * 4);
    L.nb1 = take(d.rcap);
    L.mem1 = take(uint64_t(d.rcap) * d.nw * 8);
    L.poff1 = take(uint64_t(d.rcap + 1) * 4);
    L.pred1 = take(uint64_t(d.ecap) * 4);
    // per DP row (ccsx_kernel.hip rmeta_word): band offset (bits 0-21, kMetaOff) | for a row of one or
    // two predecessors the distances - 1 of slots 0 / 1 (bits 22-25 / 26-29) and bit 30 | far flag << 31
    L.rmeta = take(uint64_t(d.rcap) * 4);
    L.spf = take(d.rcap);                              // per row: needed beyond the LDS ring
    L.sslot = take(uint64_t(d.rcap) * 4);              // per spilled row: its spill record
    L.codes = take(uint64_t(d.rcap) * kRecRow);        // cell records, 8 bits/cell, 128 B/row
    L.dsl = take(uint64_t(d.rcap) * kRecRow);          // per row: tag plane, escape distances (far rows: word 0 = far record)
    L.spill = take(uint64_t(d.scap) * (kW * 8 + 16));  // spilled rows: H, D, band offset, row-max key
    L.rrec = take(uint64_t(d.rcap) * 8);               // per row: {info, the predecessors' tag bytes} for the DP prefetch
    L.ev = take(uint64_t(d.lcap) * 4);
    L.tgt = take(uint64_t(d.lcap) * 4);
    L.ipt = take(uint64_t(d.lcap) * 4);
    L.iinf = take(d.lcap);
    L.ifix = take(uint64_t(d.lcap) * 4);
    L.cnt = take(uint64_t(d.rcap + 1) * 4);
    L.fixf = take(d.rcap + 1);
    L.addp = take(uint64_t(d.rcap) * 4);
    L.cntn = take(uint64_t(d.rcap + 1) * 4);
    L.colof = take(uint64_t(d.rcap) * 4);
    L.cons = take(d.rcap);
    L.cmask = take(uint64_t(d.rcap) * d.nw * 8);
    L.colrow = take(uint64_t(d.rcap + 1) * 4);
    L.rdoff = take(uint64_t(d.n) * 4);
    L.rdlen = take(uint64_t(d.n) * 4);
    L.rfirst = take(uint64_t(d.n) * 4);
    L.rlast = take(uint64_t(d.n) * 4);
    L.rfc = take(uint64_t(d.n) * 4);
    L.rlc = take(uint64_t(d.n) * 4);
    L.ext = take(zext_bytes(d, kExtEnd));
    L.total = o;
}

// Capacities for a ZMW with segment lengths summing to S, longest segment
// lmax, n segments.  Full caps are exact upper bounds for rows and edges
// (SPEC.md §5: each read base creates at most one node and one in-edge).
// Tight caps (the default launch) size the DP/graph arrays for the graphs a
// ZMW really builds -- rows ~ window length x (1 + error rate x reads) -- at
// a fraction of the memory; every cap is checked on the device (kErrRows,
// kErrEdges, kErrSpill) and ccsx_gpu_run re-runs a ZMW that hits
// one with full caps.  tight_rows overrides the tight row cap (tests).
// shred_win: the ZMW runs the shredded loop (main.c:541-641) with pushed
// windows of at most shred_win bases (the LDS read buffer of a tight-cap
// slice; a longer window fails the ZMW and it is re-run uncapped), whose POAs
// are of 2 kb windows (+2 kb per missed breakpoint) rather than whole
// segments, so the tight row cap follows the window, not the segment (rows ~
// window x (1 + ~0.07 reads): 3 x 4,096 + 4,096 covers 4 kb windows of up to
// ~40 reads).  0: not shredded.  The output slab: S + 16 bytes bound any
// consensus (one base per column, columns <= S); tight caps hold 2 x the
// longest segment + 1,024 (a CCS is about one insert long; kErrOut re-runs
// the ZMW uncapped), tight_out overriding (tests); tight_far overrides the
// far slot records' tight row count (tests).
CCSX_HD inline void zcaps(ZmwDesc &d, uint64_t S, uint32_t lmax, uint32_t n, bool full = true,
                          uint32_t tight_rows = 0, uint32_t shred_win = 0, uint32_t tight_out = 0,
                          uint32_t tight_far = 0)
{
    d.n = n;
    d.rcap = uint32_t(S + 16);
    d.ecap = uint32_t(S + n + 16);
    d.scap = d.rcap / 4 + 64;
    if (!full) {
        const uint64_t lw = shred_win && lmax > shred_win ? shred_win : lmax;
        uint64_t r = tight_rows ? tight_rows : 3ull * lw + 4096;
        if (r < S) {
            d.rcap = uint32_t(r + 16);
            d.ecap = 2 * d.rcap;
        }
        d.scap = d.rcap / 32 + 64;
    }
    d.lcap = lmax + 16;
    d.nw = (n + 63) / 64 ? (n + 63) / 64 : 1;
    // far rows' slot records: every row (full caps), else 1 in 16 (config E
    // 0.02 %, D 0.87 % of DP rows are far); more fail the ZMW with kErrSpill
    // and it is re-run with full caps
    d.wcap = full ? d.rcap : tight_far ? tight_far : d.rcap / 16 + 64;
    d.outcap = uint32_t(S + 16);
    if (!full) {
        const uint64_t oc = tight_out ? tight_out : 2ull * lmax + 1024;
        if (oc < d.outcap) d.outcap = uint32_t(oc);
    }
}

struct KArgs {
    const uint8_t *seq;
    const uint32_t *soff;  // segment offset relative to the ZMW's seq_off
    const uint32_t *slen;
    const ZmwDesc *desc;
    const uint32_t *order;  // workgroup -> ZMW index: most expensive first (host-sorted)
    uint8_t *ws;
    uint8_t *out;
    uint8_t *msa;
    uint32_t *out_len;
    uint32_t *ncols;
    int32_t *status;
    unsigned long long *cells;
    int32_t mode;
    uint32_t nzmw;
    uint32_t lds_read_words;    // 0: the HBM-read kernel instance (read and cursors in the workspace)
    uint32_t lds_nmax;
    unsigned long long *prof;  // optional: kProfSlots shader-clock counters per ZMW (diagnostics)
    uint32_t *bplog;           // optional: per-round breakpoint log (main.c:619-620, ZmwDesc::bp_off)
    uint8_t *qual;             // optional: a quality byte (0..kQMax, not ASCII) per CCS byte, same offsets as out
    uint32_t *pstat;           // optional: kPassWords words per segment at (ZmwDesc::seg0 + k) * kPassWords (SPEC.md §10)
    uint32_t *bmap;            // optional: a map word per pushed base (SPEC.md §11); the ZMW's segments back to back at bmoff[zmw]
    const uint64_t *bmoff;     // with bmap: per ZMW, the word offset of its map (the pushed bases of the ZMWs before it)
    uint8_t *pile;             // optional: kPuBytes per CCS byte at (ZmwDesc::out_off + offset) * kPuBytes (SPEC.md §12)
    const uint8_t *srev;       // optional, read with pile and bys: a strand flag per segment at ZmwDesc::seg0 + k (null: all forward)
    uint8_t *kin;              // optional: kKnBytes per CCS byte at (ZmwDesc::out_off + offset) * kKnBytes (SPEC.md §13); needs bmoff
    const uint8_t *kipd;       // with kin: an ipd code per pushed base, the map's index space (bmoff[zmw] + the base's entry)
    const uint8_t *kpw;        // with kin: a pw code per pushed base, likewise
    const uint8_t *ksrev;      // with kin: a kinetics strand byte (kKnRev | kKnNone) per segment at ZmwDesc::seg0 + k
    // optional: the by-strand plane (SPEC.md §14): the two lengths (forward, reverse) of ZMW i in words 2 i and
    // 2 i + 1, and behind the nzmw pairs four slabs of ZmwDesc::outcap bytes per ZMW at 8 nzmw + 4 ZmwDesc::out_off:
    // the forward strand's bases and qualities, then the reverse strand's
    uint8_t *bys;
};

// phase counters written when KArgs::prof != nullptr
enum ProfSlot { kPfTotal = 0, kPfLoad, kPfDp, kPfTrace, kPfMerge, kPfColumns, kPfShred, kPfRows,
                kPfRowA, kPfRowB, kPfRowC, kPfRowD, kPfRowE, kPfFlush, kPfSpare0, kPfSpare1,
                // two-wave DP (diagnostic build): wave 0 / wave 1 busy and barrier-wait
                // cycles, rows through the two-wave and the single-wave DP
                kPfAbusy, kPfAwait, kPfBbusy, kPfBwait, kPfTwRows, kPfSwRows, kPfSpare2, kPfSpare3,
                // traceback (diagnostic build): cycles of probe steps, plain MPRED steps,
                // D / I runs, block switches; number of block switches
                kPfTbProbe, kPfTbStep, kPfTbDI, kPfTbSwitch, kPfTbNsw,
                // placement: HW_ID | XCC_ID << 32 of waves 0, 1, 2; start / end on
                // the constant-rate s_memrealtime clock
                kPfHw0, kPfHw1, kPfHw2, kPfStartRt, kPfEndRt,
                // wave 0 fast rows (diagnostic build): head, body to the scan,
                // scan to end; number of fast rows
                kPfAHead, kPfABody, kPfATail, kPfAFast,
                // wave 0 cold rows by kind (far, chain moved 0..2, one
                // predecessor, two, other; spill rows; rows on the register
                // path for predecessors r-1 / r-2): cycles, then counts
                kPfCold0, kPfCold1, kPfCold2, kPfCold3, kPfCold4, kPfCold5, kPfCold6,
                kPfColdN0, kPfColdN1, kPfColdN2, kPfColdN3, kPfColdN4, kPfColdN5, kPfColdN6,
                // traceback (diagnostic build): insertion steps / runs, deletion steps / runs
                kPfTbIsteps, kPfTbIruns, kPfTbDsteps, kPfTbDruns, kProfSlots };

}  // namespace ccsx
