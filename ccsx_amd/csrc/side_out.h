// side_out.h -- the engine's optional per-ZMW outputs beside the CCS (the
// "side outputs": qualities, pass records, subread-to-CCS map, strand pileup,
// consensus kinetics, per-strand consensus; SPEC.md §9-§14), each described once: what it costs, where its plane lies in
// a fetched slice, how a batch's results are gathered and how an accessor finds
// them.  No HIP here: ccsx_gpu.cpp owns the device side (DESIGN.md §14 lists
// what a further output has to touch); tools/host_sanitize.cpp drives this file
// on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "ccsx_gpu.h"
#include "ccsx_layout.h"

namespace ccsx {

enum SideOut : int { kSideQual = 0, kSidePass, kSideMap, kSidePile, kSideKin, kSideStrand, kSideCount };
typedef uint32_t SideMask;  // bit o: output o is on
constexpr SideMask side_bit(int o) { return SideMask(1) << o; }
constexpr SideMask kSideAll = side_bit(kSideCount) - 1;

static_assert(sizeof(ccsx_pass_stat) == kPassWords * 4, "ccsx_pass_stat is the kernel's record");
static_assert(sizeof(ccsx_pileup) == kPuBytes, "ccsx_pileup is the kernel's record");
static_assert(sizeof(ccsx_kinetics) == kKnBytes, "ccsx_kinetics is the kernel's record");
// the by-strand output's two length words per ZMW (forward, reverse; SPEC.md §14)
constexpr uint32_t kBysLenBytes = 8;

// One row per output.  Its plane takes per_zmw bytes per ZMW (the by-strand
// output's two lengths, at the plane's start) + per_slab bytes per byte of the
// output slab + per_seg per segment + per_base per pushed base; flags_per_seg
// more bytes per segment are an input of its own (the strand flags of the
// pileup and of the by-strand output, the kinetics' strand bytes), copied back
// behind the plane; in_per_base more bytes
// per pushed base are an input that stays on the device (the kinetics' two code
// planes): they count in every device size (side_need_of), not in the fetched
// slice.
struct SideInfo {
    uint32_t per_slab, per_seg, per_base, flags_per_seg, in_per_base, per_zmw;
    bool in_out;         // the plane lies directly behind the CCS plane in the output buffer and is
                         // fetched with it, at the CCS's offsets (else: a device buffer of its own)
    const char *off;     // the accessor's refusal of a batch that ran without the output
    const char *failed;  // ... and of a ZMW without a result (null: it reads as length 0)
};
constexpr SideInfo kSide[kSideCount] = {
    {1, 0, 0, 0, 0, 0, true, "that batch ran with quality off (ccsx_gpu_set_quality)", nullptr},
    {0, kPassWords * 4, 0, 0, 0, 0, false, "that batch ran with pass statistics off (ccsx_gpu_set_pass_stats)",
     "that ZMW failed: it has no pass statistics"},
    {0, 0, 4, 0, 0, 0, false, "that batch ran with the base map off (ccsx_gpu_set_base_map)",
     "that ZMW failed: it has no base map"},
    {kPuBytes, 0, 0, 1, 0, 0, false, "that batch ran with the pileup off (ccsx_gpu_set_pileup)",
     "that ZMW failed: it has no pileup"},
    {kKnBytes, 0, 0, 1, 2, 0, false, "that batch ran with kinetics off (ccsx_gpu_set_kinetics)",
     "that ZMW failed: it has no kinetics"},
    // (bases and qualities of two strands: four bytes per byte of the output slab)
    {4, 0, 0, 1, 0, kBysLenBytes, false, "that batch ran with the by-strand output off (ccsx_gpu_set_by_strand)",
     "that ZMW failed: it has no strand consensus"},
};

// Bytes of output o's plane and, with its flags, the bytes it takes in a
// fetched slice; with its device-only input (side_input) the bytes it adds to a
// ZMW (nz = 1, its output slab, segments, pushed bases) or to a slice of nz ZMWs
// (their sums)
inline uint64_t side_plane(int o, uint64_t nz, uint64_t slab, uint64_t nseg, uint64_t nbase)
{
    return kSide[o].per_zmw * nz + kSide[o].per_slab * slab + kSide[o].per_seg * nseg + kSide[o].per_base * nbase;
}
inline uint64_t side_bytes(int o, uint64_t nz, uint64_t slab, uint64_t nseg, uint64_t nbase)
{
    return side_plane(o, nz, slab, nseg, nbase) + kSide[o].flags_per_seg * nseg;
}
inline uint64_t side_input(int o, uint64_t nbase) { return uint64_t(kSide[o].in_per_base) * nbase; }
inline uint64_t side_bytes_of(SideMask m, uint64_t nz, uint64_t slab, uint64_t nseg, uint64_t nbase)
{
    uint64_t b = 0;
    for (int o = 0; o < kSideCount; ++o)
        if (m & side_bit(o)) b += side_bytes(o, nz, slab, nseg, nbase);
    return b;
}
// ... and what the outputs of m add to the device bytes of a ZMW or a slice
inline uint64_t side_need_of(SideMask m, uint64_t nz, uint64_t slab, uint64_t nseg, uint64_t nbase)
{
    uint64_t b = side_bytes_of(m, nz, slab, nseg, nbase);
    for (int o = 0; o < kSideCount; ++o)
        if (m & side_bit(o)) b += side_input(o, nbase);
    return b;
}

// Where a slice's planes lie in its host output buffer: the CCS plane (the
// output slabs) at 0, an in_out plane directly behind it, every other one 8-byte
// aligned behind that, its flags behind its records.
struct SideLayout {
    SideMask mask = 0;
    uint64_t plane[kSideCount] = {};  // bytes of the plane (its device buffer, or its part of the output buffer)
    uint64_t bytes[kSideCount] = {};  // ... and with the flags behind it
    uint64_t off[kSideCount] = {};    // offset in the host buffer
    uint64_t out_dev = 0;             // bytes of the device output buffer: the CCS plane and the in_out planes
    uint64_t total = 0;               // bytes of the host buffer
    bool has(int o) const { return (mask & side_bit(o)) != 0; }
    uint64_t nzmw = 0;                // ZMWs of the slice
    void plan(SideMask m, uint64_t nz, uint64_t slab, uint64_t nseg, uint64_t nbase)
    {
        mask = m;
        nzmw = nz;
        out_dev = total = slab;
        for (int o = 0; o < kSideCount; ++o) {
            plane[o] = bytes[o] = off[o] = 0;
            if (!has(o)) continue;
            plane[o] = side_plane(o, nz, slab, nseg, nbase);
            bytes[o] = side_bytes(o, nz, slab, nseg, nbase);
            off[o] = kSide[o].in_out ? total : (total + 7) & ~uint64_t(7);
            total = off[o] + bytes[o];
            if (kSide[o].in_out) out_dev = total;
        }
    }
};
// (an in_out plane behind an aligned one would not be fetched with the CCS)
static_assert(kSide[0].in_out && !kSide[1].in_out && !kSide[2].in_out && !kSide[3].in_out && !kSide[4].in_out &&
                  !kSide[5].in_out,
              "in_out planes come first");

// One ZMW's results where they lie, in a fetched slice or a gathered batch; the
// planes of outputs that are off are null
struct SideRec {
    bool ok = false;                  // it has a result (status 0)
    uint32_t len = 0, nseg = 0;       // CCS bytes (0 without a result), segments
    const uint8_t *ccs = nullptr;
    const uint8_t *qual = nullptr;    // len bytes
    const uint32_t *pass = nullptr;   // kPassWords per segment
    const uint32_t *map = nullptr;    // a word per pushed base, the segments back to back
    const uint32_t *seg_len = nullptr;  // with map: nseg lengths
    const uint32_t *seg_at = nullptr;   // with map: nseg word offsets into map (null: the lengths' running sum)
    const ccsx_pileup *pile = nullptr;  // len records
    const ccsx_kinetics *kin = nullptr;  // len records
    // the strand consensuses (SPEC.md §14), forward then reverse: slen[s] bases and as many quality bytes
    const uint8_t *sseq[2] = {nullptr, nullptr}, *squal[2] = {nullptr, nullptr};
    uint32_t slen[2] = {0, 0};
    // segment k of the map
    const uint32_t *map_seg(uint32_t k) const
    {
        if (seg_at) return map + seg_at[k];
        uint64_t at = 0;
        for (uint32_t j = 0; j < k; ++j) at += seg_len[j];
        return map + at;
    }
};

// A fetched slice: its host buffer and the host tables that index it
struct SideView {
    const SideLayout *lay = nullptr;
    const uint8_t *h_out = nullptr;
    size_t nz = 0;
    const ZmwDesc *desc = nullptr;
    const uint32_t *seg_len = nullptr;   // per segment of the slice (ZmwDesc::seg0)
    const uint64_t *map_off = nullptr;   // with the map: per ZMW, the word offset of its map
    const int32_t *status = nullptr;
    const uint32_t *out_len = nullptr;
    SideMask enabled() const { return lay->mask; }
    size_t size() const { return nz; }
    SideRec rec(size_t i) const
    {
        const ZmwDesc &d = desc[i];
        SideRec r;
        r.ok = status[i] == 0;
        r.len = r.ok ? out_len[i] : 0;
        r.nseg = d.n;
        r.ccs = h_out + d.out_off;
        if (lay->has(kSideQual)) r.qual = h_out + lay->off[kSideQual] + d.out_off;
        if (lay->has(kSidePass))
            r.pass = reinterpret_cast<const uint32_t *>(h_out + lay->off[kSidePass]) + size_t(d.seg0) * kPassWords;
        if (lay->has(kSideMap)) {
            r.map = reinterpret_cast<const uint32_t *>(h_out + lay->off[kSideMap]) + map_off[i];
            r.seg_len = seg_len + d.seg0;
        }
        if (lay->has(kSidePile)) r.pile = reinterpret_cast<const ccsx_pileup *>(h_out + lay->off[kSidePile]) + d.out_off;
        if (lay->has(kSideKin)) r.kin = reinterpret_cast<const ccsx_kinetics *>(h_out + lay->off[kSideKin]) + d.out_off;
        if (lay->has(kSideStrand)) {
            // the pairs of lengths, then per ZMW four slabs of its outcap bytes
            const uint8_t *pl = h_out + lay->off[kSideStrand];
            const uint8_t *zp = pl + uint64_t(kBysLenBytes) * lay->nzmw + 4 * d.out_off;
            for (int s = 0; s < 2; ++s) {
                r.slen[s] = r.ok ? reinterpret_cast<const uint32_t *>(pl)[2 * i + s] : 0;
                r.sseq[s] = zp + size_t(2 * s) * d.outcap;
                r.squal[s] = zp + size_t(2 * s + 1) * d.outcap;
            }
        }
        return r;
    }
};

// The gathered results of one ccsx_gpu_run call or one collected batch, per ZMW
// of the call in input order: the CCS strings and, for every output of `mask`,
// its payload.  Qualities, pileup and kinetics records lie at the CCS's offsets.
struct Gathered {
    struct At {
        uint64_t ccs = 0, pass = 0, map = 0, seg = 0;  // offsets into arena (qual, pile, kin), pass, map, seg_len (seg_at)
        uint64_t str = 0;  // ... and into sseq / squal: the forward strand's bytes, the reverse strand's behind them
        uint32_t len = 0, nseg = 0, slen[2] = {0, 0};
        bool ok = false;
    };
    SideMask mask = 0;
    std::vector<At> at;               // per ZMW
    std::vector<uint8_t> arena, qual, sseq, squal;
    std::vector<uint32_t> pass, map;
    std::vector<uint32_t> seg_len, seg_at;  // per gathered segment of the map: entries, word offset in its ZMW's map
    std::vector<ccsx_pileup> pile;
    std::vector<ccsx_kinetics> kin;
    SideMask enabled() const { return mask; }
    bool has(int o) const { return (mask & side_bit(o)) != 0; }
    size_t size() const { return at.size(); }
    void reset(size_t nz, SideMask m)
    {
        mask = m;
        at.assign(nz, At{});
        arena.clear(), qual.clear(), pass.clear(), map.clear(), seg_len.clear(), seg_at.clear(), pile.clear(), kin.clear();
        sseq.clear(), squal.clear();
    }
    // one growth per slice of `add` CCS bytes, not one per ZMW's append (~150
    // MB for a 10k-ZMW slice of 15 kb inserts)
    void grow(size_t add)
    {
        arena.reserve(arena.size() + add);
        if (has(kSideQual)) qual.reserve(qual.size() + add);
    }
    // ZMW g of the call: the result r of a slice fetched with this mask
    void put(size_t g, const SideRec &r)
    {
        At &a = at[g];
        a.ok = true;
        a.len = r.len, a.nseg = r.nseg;
        a.ccs = arena.size();
        arena.insert(arena.end(), r.ccs, r.ccs + r.len);
        if (has(kSideQual)) qual.insert(qual.end(), r.qual, r.qual + r.len);
        if (has(kSidePass)) {
            a.pass = pass.size();
            pass.insert(pass.end(), r.pass, r.pass + size_t(r.nseg) * kPassWords);
        }
        if (has(kSideMap)) {
            a.map = map.size(), a.seg = seg_len.size();
            uint32_t tot = 0;  // (a ZMW pushes fewer than 2^30 bases)
            for (uint32_t k = 0; k < r.nseg; ++k) {
                seg_at.push_back(tot);
                seg_len.push_back(r.seg_len[k]);
                tot += r.seg_len[k];
            }
            map.insert(map.end(), r.map, r.map + tot);
        }
        if (has(kSidePile)) pile.insert(pile.end(), r.pile, r.pile + r.len);
        if (has(kSideKin)) kin.insert(kin.end(), r.kin, r.kin + r.len);
        if (has(kSideStrand)) {
            a.str = sseq.size();
            for (int s = 0; s < 2; ++s) {
                a.slen[s] = r.slen[s];
                sseq.insert(sseq.end(), r.sseq[s], r.sseq[s] + r.slen[s]);
                squal.insert(squal.end(), r.squal[s], r.squal[s] + r.slen[s]);
            }
        }
    }
    // ZMW g is reported as failed after all: without a result in every output
    void drop(size_t g) { at[g].ok = false, at[g].len = 0, at[g].slen[0] = at[g].slen[1] = 0; }
    const char *ccs(size_t g) const { return reinterpret_cast<const char *>(arena.data() + at[g].ccs); }
    SideRec rec(size_t g) const
    {
        const At &a = at[g];
        SideRec r;
        r.ok = a.ok;
        r.len = a.len, r.nseg = a.nseg;
        r.ccs = arena.data() + a.ccs;
        if (has(kSideQual)) r.qual = qual.data() + a.ccs;
        if (has(kSidePass)) r.pass = pass.data() + a.pass;
        if (has(kSideMap)) r.map = map.data() + a.map, r.seg_len = seg_len.data() + a.seg, r.seg_at = seg_at.data() + a.seg;
        if (has(kSidePile)) r.pile = pile.data() + a.ccs;
        if (has(kSideKin)) r.kin = kin.data() + a.ccs;
        if (has(kSideStrand))
            for (int s = 0; s < 2; ++s) {
                const uint64_t o = a.str + (s ? a.slen[0] : 0);
                r.slen[s] = a.slen[s], r.sseq[s] = sseq.data() + o, r.squal[s] = squal.data() + o;
            }
        return r;
    }
};

// Output o of ZMW `zmw` in a gathered batch or a fetched slice: null and r, or
// the accessor's refusal.  A ZMW without a result is refused unless the output
// has no `failed` text: then r.ok is false and r.len 0.
template <class Src>
inline const char *side_find(const Src &src, int o, size_t zmw, SideRec &r)
{
    if (!(src.enabled() & side_bit(o))) return kSide[o].off;
    if (zmw >= src.size()) return "ZMW index beyond the batch";
    r = src.rec(zmw);
    return r.ok ? nullptr : kSide[o].failed;
}

}  // namespace ccsx
