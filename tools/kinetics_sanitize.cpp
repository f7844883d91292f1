// kinetics_sanitize.cpp -- drives the host C++ of the consensus kinetics
// (SPEC.md §13) under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU:
// the BAM aux parser of the ingest (at block sizes down to 1 byte, on records
// with well-formed, missing, miscounted and cut-short ip / pw arrays),
// ccsx_prepare_apply_kin, ccsx_kinetics_tags, and the kinetics output's
// bookkeeping in side_out.h under all 32 masks of the first five outputs.  tests/test_kinetics_sanitize.py
// compiles it with the host sources it needs (no HIP code is involved).
//   kinetics_sanitize FILE.bam ...   prints one line per ZMW read
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ccsx_host.h"
#include "ccsx_seqio.h"
#include "../ccsx_amd/csrc/side_out.h"

static uint32_t crc(const void *p, size_t n) { return (uint32_t)crc32(0, static_cast<const unsigned char *>(p), (uInt)n); }

// side_out.h with the fifth output: sizes (the per-base input counts on the
// device only), the plane's place in a slice, gathering and lookup, under every
// subset of the first five outputs (tools/host_sanitize.cpp walks the later ones)
static int side_outputs()
{
    using namespace ccsx;
    struct Z {
        std::vector<uint32_t> lens;
        uint32_t outcap, status;
    };
    const std::vector<Z> zs = {{{7, 5, 9}, 40, 0}, {{}, 16, 0}, {{4, 0}, 33, 0}, {{11}, 24, kErrOut}, {{3, 3, 3, 2}, 32, 0}};
    const size_t nz = zs.size();
    const SideMask five = side_bit(kSideKin + 1) - 1;
    for (SideMask m = 0; m <= five; ++m) {
        std::vector<ZmwDesc> desc(nz);
        std::vector<uint32_t> seg_len, out_len(nz);
        std::vector<uint64_t> map_off(nz);
        std::vector<int32_t> status(nz);
        uint64_t slab = 0, nbase = 0, need = 0;
        for (size_t i = 0; i < nz; ++i) {
            uint64_t S = 0;
            for (uint32_t l : zs[i].lens) S += l;
            desc[i].seg0 = (uint32_t)seg_len.size(), desc[i].n = (uint32_t)zs[i].lens.size();
            desc[i].out_off = slab, desc[i].outcap = zs[i].outcap;
            map_off[i] = nbase, status[i] = (int32_t)zs[i].status, out_len[i] = zs[i].outcap - 3;
            need += side_need_of(m, 1, zs[i].outcap, zs[i].lens.size(), S);
            if (side_need_of(m, 1, zs[i].outcap, zs[i].lens.size(), S) -
                    side_need_of(m & ~side_bit(kSideKin), 1, zs[i].outcap, zs[i].lens.size(), S) !=
                ((m & side_bit(kSideKin)) ? 8ull * zs[i].outcap + 2 * S + zs[i].lens.size() : 0ull))
                return 70;
            seg_len.insert(seg_len.end(), zs[i].lens.begin(), zs[i].lens.end());
            slab += zs[i].outcap, nbase += S;
        }
        if (side_need_of(m, nz, slab, seg_len.size(), nbase) != need) return 71;
        if (side_need_of(m, nz, slab, seg_len.size(), nbase) !=
            side_bytes_of(m, nz, slab, seg_len.size(), nbase) + ((m & side_bit(kSideKin)) ? 2 * nbase : 0))
            return 72;
        SideLayout L;
        L.plan(m, nz, slab, seg_len.size(), nbase);
        if (L.has(kSideKin) && (L.plane[kSideKin] != slab * kKnBytes || L.bytes[kSideKin] != L.plane[kSideKin] + seg_len.size() ||
                                L.off[kSideKin] % 8 || L.off[kSideKin] + L.bytes[kSideKin] != L.total))
            return 73;
        std::vector<uint8_t> h(L.total);
        for (size_t j = 0; j < h.size(); ++j) h[j] = uint8_t(j * 37 + m * 5 + 3);
        const SideView v{&L, h.data(), nz, desc.data(), seg_len.data(), map_off.data(), status.data(), out_len.data()};
        Gathered G;
        G.reset(nz, m);
        for (size_t i = 0; i < nz; ++i)
            if (!status[i]) G.put(nz - 1 - i, v.rec(i));
        for (size_t i = 0; i <= nz; ++i) {
            SideRec r[2];
            const char *e[2] = {side_find(v, kSideKin, i, r[0]), side_find(G, kSideKin, i < nz ? nz - 1 - i : i, r[1])};
            for (int k = 0; k < 2; ++k) {
                if (!(m & side_bit(kSideKin))) {
                    if (e[k] != kSide[kSideKin].off) return 74;
                } else if (i == nz) {
                    if (!e[k] || r[k].kin) return 75;
                } else if (status[i]) {
                    if (e[k] != kSide[kSideKin].failed || r[k].len) return 76;
                } else if (e[k] || r[k].len != out_len[i] ||
                           memcmp(r[k].kin, h.data() + L.off[kSideKin] + desc[i].out_off * kKnBytes, size_t(r[k].len) * kKnBytes)) {
                    return 77;
                }
            }
        }
    }
    printf("side outputs %d masks\n", (int)five + 1);
    return 0;
}

int main(int argc, char **argv)
{
    // 1. the codec: every byte and the values around the group edges
    for (uint32_t b = 0; b < 256; ++b)
        if (ccsx_kin_code(ccsx_kin_frames((uint8_t)b)) != b) return 10;
    for (uint32_t f : {0u, 63u, 64u, 191u, 446u, 447u, 952u, 953u, 65535u, 0xFFFFFFFFu}) (void)ccsx_kin_code(f);
    // 2. the aux parser, ccsx_prepare_apply_kin and the formatter on what it read
    for (int a = 1; a < argc; ++a) {
        const std::string path(argv[a]);
        for (const char *blk : {"1", "7", "64", "4096", ""}) {
            if (*blk) setenv("CCSX_INGEST_BLOCK", blk, 1);
            else unsetenv("CCSX_INGEST_BLOCK");
            ccsx_reader *r = ccsx_reader_open(path.c_str(), 1);
            if (!r) return 3;
            const char *movie, *hole, *seqs;
            const uint32_t *lens;
            const uint8_t *ipd, *pw;
            int l;
            while ((l = ccsx_reader_next_kin(r, &movie, &hole, &seqs, &lens, &ipd, &pw)) >= 0) {
                size_t tot = 0;
                for (int k = 0; k < l; ++k) tot += lens[k];
                if ((ipd == nullptr) != (pw == nullptr)) return 11;
                if (*blk == 0)
                    printf("%s %s/%s %d %zu %08x %08x %08x\n", path.c_str(), movie, hole, l, tot, crc(seqs, tot), ipd ? crc(ipd, tot) : 0u,
                           pw ? crc(pw, tot) : 0u);
                std::string s(seqs, tot);
                // (exactly tot bytes each: a reversal past a segment's end is past the allocation)
                std::vector<uint8_t> pi(ipd ? ipd : reinterpret_cast<const uint8_t *>(seqs), (ipd ? ipd : reinterpret_cast<const uint8_t *>(seqs)) + tot);
                std::vector<uint8_t> pp(pw ? pw : reinterpret_cast<const uint8_t *>(seqs), (pw ? pw : reinterpret_cast<const uint8_t *>(seqs)) + tot);
                const std::vector<uint8_t> i0 = pi, p0 = pp;
                std::vector<uint32_t> off(l), len(l);
                std::vector<uint8_t> rev(l);
                const uint32_t ns = ccsx_prepare_apply_kin(&s[0], pi.data(), ipd ? pp.data() : nullptr, lens, (uint32_t)l, off.data(),
                                                           len.data(), rev.data());
                for (uint32_t k = 0; k < ns; ++k) {
                    if (off[k] + (uint64_t)len[k] > tot) return 12;
                    for (uint32_t j = 0; j < len[k]; ++j) {
                        const uint32_t from = rev[k] ? off[k] + len[k] - 1 - j : off[k] + j;
                        if (pi[off[k] + j] != i0[from] || (ipd && pp[off[k] + j] != p0[from])) return 13;
                    }
                }
                // the planes as records: the formatter's two passes agree, a short buffer is cut and terminated
                const uint32_t nrec = (uint32_t)(tot / sizeof(ccsx_kinetics) < 300 ? tot / sizeof(ccsx_kinetics) : 300);
                std::vector<ccsx_kinetics> rec(nrec);
                if (nrec) memcpy(rec.data(), pi.data(), size_t(nrec) * sizeof(ccsx_kinetics));
                const long n = ccsx_kinetics_tags(rec.data(), nrec, nullptr, 0);
                std::vector<char> buf((size_t)n + 1);
                if (ccsx_kinetics_tags(rec.data(), nrec, buf.data(), buf.size()) != n || strlen(buf.data()) != (size_t)n) return 14;
                std::vector<char> cut(8);
                if (ccsx_kinetics_tags(rec.data(), nrec, cut.data(), cut.size()) != n || strlen(cut.data()) != 7) return 15;
            }
            ccsx_reader_close(r);
        }
    }
    // 3. the kinetics output in side_out.h, every subset of the outputs
    if (const int r = side_outputs()) return r;
    printf("ok\n");
    return 0;
}
