// host_sanitize.cpp -- drives the host C++ of the product (ingest, seqio C-ABI,
// ccs_prepare, the pairwise aligner, the synthetic source, the dispatch
// partitioner, the engine's optional-output bookkeeping of side_out.h) under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU.
// tests/test_sanitize.py compiles it together with those sources
// (-fsanitize=address,undefined; no HIP code is involved) and runs it on the
// golden ingest fixtures and synthetic ZMWs.
//   host_sanitize FIXTURE:is_bam ...   prints one line per ZMW read
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "ccsx_host.h"
#include "ccsx_seqio.h"
#include "../ccsx_amd/csrc/side_out.h"  // (by path: it and ccsx_layout.h beside it are not on the include path of this build)

static uint32_t crc(const char *p, size_t n) { return (uint32_t)crc32(0, reinterpret_cast<const unsigned char *>(p), (uInt)n); }

// side_out.h on synthetic slices of 0, 1 and 5 ZMWs under all 64 masks: a ZMW
// without a segment, one with an odd output slab (the slice's slabs then end off
// a multiple of 8), one with an empty segment, one failed.  Returns 0 or the
// number of the check that failed.
static int side_outputs()
{
    using namespace ccsx;
    struct Z {
        std::vector<uint32_t> lens;
        uint32_t outcap, status;
    };
    const std::vector<Z> five = {{{7, 5, 9}, 40, 0}, {{}, 16, 0}, {{4, 0}, 33, 0}, {{11}, 24, kErrOut}, {{3, 3, 3, 2}, 32, 0}};
    const std::vector<Z> one = {five[2]};
    const size_t perm5[5] = {2, 4, 0, 3, 1};
    const size_t align[kSideCount] = {1, alignof(uint32_t), alignof(uint32_t), alignof(ccsx_pileup), alignof(ccsx_kinetics),
                                      alignof(uint32_t)};
    for (SideMask m = 0; m <= kSideAll; ++m)
        for (const std::vector<Z> *zs : {(const std::vector<Z> *)nullptr, &one, &five}) {
            const size_t nz = zs ? zs->size() : 0;
            // the slice's tables, as stage_slot lays them out
            std::vector<ZmwDesc> desc(nz);
            std::vector<uint32_t> seg_len, out_len(nz);
            std::vector<uint64_t> map_off(nz);
            std::vector<int32_t> status(nz);
            uint64_t slab = 0, nbase = 0, per_zmw[kSideCount] = {};
            for (size_t i = 0; i < nz; ++i) {
                const Z &z = (*zs)[i];
                uint64_t S = 0;
                for (uint32_t l : z.lens) S += l;
                desc[i].seg0 = (uint32_t)seg_len.size();
                desc[i].n = (uint32_t)z.lens.size();
                desc[i].out_off = slab;
                desc[i].outcap = z.outcap;
                map_off[i] = nbase;
                status[i] = (int32_t)z.status;
                out_len[i] = z.outcap - 3;
                for (int o = 0; o < kSideCount; ++o) per_zmw[o] += side_bytes(o, 1, z.outcap, z.lens.size(), S);
                seg_len.insert(seg_len.end(), z.lens.begin(), z.lens.end());
                slab += z.outcap, nbase += S;
            }
            if (nz && slab % 8 == 0) return 50;
            // sizes: a slice's is the sum of its ZMWs', per output and for the mask
            uint64_t sum = 0;
            for (int o = 0; o < kSideCount; ++o) {
                if (side_bytes(o, nz, slab, seg_len.size(), nbase) != per_zmw[o]) return 51;
                if (m & side_bit(o)) sum += per_zmw[o];
            }
            if (side_bytes_of(m, nz, slab, seg_len.size(), nbase) != sum) return 52;
            // layout: the planes in order, none overlapping, each aligned for its
            // elements, less than 8 bytes of padding before each; the total is
            // the CCS plane, the enabled outputs and that padding
            SideLayout L;
            L.plan(m, nz, slab, seg_len.size(), nbase);
            uint64_t end = slab, pad = 0;
            for (int o = 0; o < kSideCount; ++o) {
                if (!(m & side_bit(o))) {
                    if (L.has(o) || L.bytes[o] || L.plane[o]) return 53;
                    continue;
                }
                if (!L.has(o) || L.off[o] < end || L.off[o] - end >= 8 || L.off[o] % align[o]) return 54;
                if (L.bytes[o] != side_bytes(o, nz, slab, seg_len.size(), nbase) || L.plane[o] > L.bytes[o]) return 55;
                if (kSide[o].in_out && (L.off[o] != end || L.out_dev != L.off[o] + L.plane[o])) return 56;
                pad += L.off[o] - end;
                end = L.off[o] + L.bytes[o];
            }
            if (L.total != end || L.total != slab + sum + pad || L.out_dev < slab) return 57;
            // fake planes: every byte derived from its index (exactly L.total
            // bytes, so a read past a plane's end is one past the allocation)
            std::vector<uint8_t> h(L.total);
            for (size_t j = 0; j < h.size(); ++j) h[j] = uint8_t(j * 131 + m * 7 + 1);
            // the by-strand plane's lengths are read as lengths: one strand fills
            // its slab to the last byte, the other is empty or a byte long
            auto strand_len = [&](size_t i, int s) { return s == int(i & 1) ? desc[i].outcap : uint32_t(i % 3 == 0); };
            if (L.has(kSideStrand))
                for (size_t i = 0; i < nz; ++i)
                    for (int s = 0; s < 2; ++s) {
                        const uint32_t v = strand_len(i, s);
                        memcpy(h.data() + L.off[kSideStrand] + (2 * i + s) * 4, &v, 4);
                    }
            const SideView v{&L, h.data(), nz, desc.data(), seg_len.data(), map_off.data(), status.data(), out_len.data()};
            // gathered in a permuted input order: ZMW i of the slice is input perm[i]
            Gathered G;
            G.reset(nz, m);
            size_t add = 0;
            for (size_t i = 0; i < nz; ++i) add += status[i] ? 0 : out_len[i];
            G.grow(add);
            std::vector<size_t> perm(nz, 0), slice_of(nz, 0);
            for (size_t i = 0; i < nz; ++i) perm[i] = nz == 5 ? perm5[i] : i, slice_of[perm[i]] = i;
            for (size_t i = 0; i < nz; ++i)
                if (!status[i]) G.put(perm[i], v.rec(i));
            // every ZMW back through the lookup, from the gathered batch and from the slice itself
            for (int o = 0; o < kSideCount; ++o)
                for (size_t g = 0; g <= nz; ++g) {
                    SideRec r[2];
                    const char *e[2] = {side_find(G, o, g, r[0]), g < nz ? side_find(v, o, slice_of[g], r[1]) : side_find(v, o, g, r[1])};
                    for (int k = 0; k < 2; ++k) {
                        if (!(m & side_bit(o))) {
                            if (e[k] != kSide[o].off) return 58;
                            continue;
                        }
                        if (g == nz) {
                            if (!e[k] || std::string(e[k]) != "ZMW index beyond the batch") return 59;
                            continue;
                        }
                        const size_t i = slice_of[g];
                        const ZmwDesc &d = desc[i];
                        if (status[i]) {
                            if (e[k] != kSide[o].failed || r[k].ok || r[k].len) return 60;
                            continue;
                        }
                        if (e[k] || !r[k].ok || r[k].len != out_len[i] || r[k].nseg != d.n) return 61;
                        if (memcmp(r[k].ccs, h.data() + d.out_off, r[k].len)) return 62;
                        if (o == kSideQual && memcmp(r[k].qual, h.data() + L.off[o] + d.out_off, r[k].len)) return 63;
                        if (o == kSidePass &&
                            memcmp(r[k].pass, h.data() + L.off[o] + size_t(d.seg0) * kPassWords * 4, size_t(d.n) * kPassWords * 4))
                            return 64;
                        if (o == kSidePile && memcmp(r[k].pile, h.data() + L.off[o] + d.out_off * kPuBytes, size_t(r[k].len) * kPuBytes))
                            return 65;
                        if (o == kSideStrand)
                            for (int s = 0; s < 2; ++s) {
                                const uint8_t *zp = h.data() + L.off[o] + kBysLenBytes * nz + 4 * d.out_off;
                                if (r[k].slen[s] != strand_len(i, s)) return 69;
                                if (memcmp(r[k].sseq[s], zp + size_t(2 * s) * d.outcap, r[k].slen[s])) return 70;
                                if (memcmp(r[k].squal[s], zp + size_t(2 * s + 1) * d.outcap, r[k].slen[s])) return 71;
                            }
                        if (o == kSideMap) {
                            uint64_t at = map_off[i];
                            for (uint32_t s = 0; s < d.n; ++s) {
                                if (r[k].seg_len[s] != seg_len[d.seg0 + s]) return 66;
                                if (memcmp(r[k].map_seg(s), h.data() + L.off[o] + at * 4, size_t(seg_len[d.seg0 + s]) * 4)) return 67;
                                at += seg_len[d.seg0 + s];
                            }
                        }
                    }
                }
            // the injected fault: a gathered ZMW dropped afterwards has no result in any output
            if (nz) {
                G.drop(perm[0]);
                for (int o = 0; o < kSideCount; ++o) {
                    SideRec r;
                    if ((m & side_bit(o)) && (side_find(G, o, perm[0], r) != kSide[o].failed || r.ok || r.len || r.slen[0] || r.slen[1]))
                        return 68;
                }
            }
        }
    printf("side outputs %d masks\n", (int)kSideAll + 1);
    return 0;
}

int main(int argc, char **argv)
{
    // 1. ingest: every fixture at several block sizes (records crossing blocks)
    for (int a = 1; a < argc; ++a) {
        std::string arg(argv[a]);
        const size_t c = arg.rfind(':');
        const std::string path = arg.substr(0, c);
        const int bam = atoi(arg.c_str() + c + 1);
        for (const char *blk : {"1", "5", "64", ""}) {
            if (*blk) setenv("CCSX_INGEST_BLOCK", blk, 1);
            else unsetenv("CCSX_INGEST_BLOCK");
            ccsx_reader *r = ccsx_reader_open(path.c_str(), bam);
            if (!r) return 3;
            const char *movie, *hole, *seqs;
            const uint32_t *lens;
            // main.c step 0: a chunk ends at -1, the next one reads on, and
            // the input ends at the first chunk without a ZMW
            int l, got = 1;
            while (got) {
                got = 0;
                while ((l = ccsx_reader_next(r, &movie, &hole, &seqs, &lens)) >= 0) {
                    ++got;
                    size_t tot = 0;
                    for (int k = 0; k < l; ++k) tot += lens[k];
                    if (*blk == 0) printf("%s %s/%s %d %zu %08x\n", path.c_str(), movie, hole, l, tot, crc(seqs, tot));
                    // prepare + strand flip on what was read
                    std::string s(seqs, tot);
                    std::vector<uint32_t> off(l), len(l);
                    const uint32_t ns = ccsx_prepare_apply(&s[0], lens, (uint32_t)l, off.data(), len.data());
                    for (uint32_t k = 0; k < ns; ++k)
                        if (off[k] + (uint64_t)len[k] > tot) return 4;
                }
                if (*blk == 0) printf("%s -1\n", path.c_str());
            }
            ccsx_reader_close(r);
        }
    }
    // 2. ccs_prepare on synthetic ZMWs with abnormal subreads (random
    // truncations, adapters read through, short and empty subreads)
    std::mt19937_64 rng(7);
    for (int z = 0; z < 60; ++z) {
        const uint32_t L = 300 + (uint32_t)(rng() % 3000), passes = 3 + (uint32_t)(rng() % 9);
        std::string out((size_t)passes * (2 * L + 16) + 16, '\0');
        std::vector<uint32_t> lens(passes);
        ccsx_synth_zmw(20201104, (uint64_t)z, L, passes, &out[0], lens.data(), nullptr);
        std::string seqs;
        size_t o = 0;
        std::vector<uint32_t> l2;
        for (uint32_t k = 0; k < passes; ++k) {
            std::string sub = out.substr(o, lens[k]);
            o += lens[k];
            switch (rng() % 6) {
            case 0: sub = sub.substr(0, sub.size() / 3); break;                         // truncated
            case 1: { std::string rc = sub; ccsx_revcomp(&rc[0], (uint32_t)rc.size()); sub += rc; break; }  // palindrome
            case 2: sub.clear(); break;                                                   // empty
            default: break;
            }
            seqs += sub;
            l2.push_back((uint32_t)sub.size());
        }
        std::vector<uint32_t> off(passes), len(passes);
        std::vector<uint8_t> rev(passes);
        const uint32_t ns = ccsx_prepare(seqs.data(), l2.data(), passes, off.data(), len.data(), rev.data());
        for (uint32_t k = 0; k < ns; ++k)
            if (off[k] + (uint64_t)len[k] > seqs.size()) return 5;
        printf("prepare %d %u\n", z, ns);
    }
    // 3. the pairwise aligner on random 2-bit sequences (codes >= 4 included)
    for (int t = 0; t < 40; ++t) {
        std::vector<uint8_t> q(rng() % 3000), s(rng() % 3000);
        for (auto &x : q) x = (uint8_t)(rng() % 5);
        for (auto &x : s) x = (uint8_t)(rng() % 5);
        const ccsx_pairaln r = ccsx_pairwise(q.data(), (uint32_t)q.size(), s.data(), (uint32_t)s.size());
        if (r.qe < r.qb || r.te < r.tb) return 6;
    }
    // 4. the dispatch partitioner
    for (int t = 0; t < 50; ++t) {
        const uint32_t n = (uint32_t)(rng() % 5000);
        std::vector<uint64_t> cost(n);
        for (auto &x : cost) x = rng() % 1000000;
        std::vector<uint32_t> order(n ? n : 1), bounds(n + 1);
        const uint32_t nb = ccsx_partition(cost.data(), n, 1 + (uint32_t)(rng() % 40), 1 + (uint32_t)(rng() % 300),
                                           order.data(), bounds.data());
        if (nb > n || bounds[nb] != n) return 7;
    }
    // 5. the engine's optional outputs (side_out.h): sizes, slice layout,
    // gathering and lookup, for every subset of the outputs
    if (const int r = side_outputs()) return r;
    printf("ok\n");
    return 0;
}
