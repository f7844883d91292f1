// prepare.cpp -- ccs_prepare and the strand flip (main.c:116-453, seqio.h:120-148).
//
// Host code of the C host program; the GPU engine consumes its output.  The
// pairwise aligner that bsalign's kmer_striped_seqedit_pairwise provides to
// strand_match is un-vendored; ccsx_pairwise restates it per SPEC.md §8.
// ccs_prepare is written once, as a walk that stops where it needs
// strand_match's alignments (ccsx_prep_*): ccsx_prepare answers them with
// ccsx_pairwise on the spot, ccsx_prepare_batch (prepare_gpu.cpp) for a whole
// chunk of ZMWs at once on the device.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "ccsx_host.h"

namespace {

// seqio.h:120-137 complement table (identity outside IUPAC letters)
struct CompTable {
    unsigned char t[256];
    CompTable()
    {
        for (int i = 0; i < 256; ++i) t[i] = (unsigned char)i;
        const char *from = "ABCDGHKMNRSTUVWYabcdghkmnrstuvwy";
        const char *to = "TVGHCDMKNYSAABWRtvghcdmknysaabwr";
        for (int i = 0; from[i]; ++i) t[(unsigned char)from[i]] = (unsigned char)to[i];
    }
};
const CompTable kComp;

// bsalign dna.h base_bit_table as used by recap_base_bit_u1v (main.c:222-241)
inline uint8_t base_bit(unsigned char c)
{
    switch (c) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': case 'U': case 'u': return 3;
    default: return 4;
    }
}

// main.c:222-241: 2-bit copy, reverse = reverse complement (3 - code)
void recap(std::vector<uint8_t> &v, const char *buf, size_t len, bool reverse)
{
    v.resize(len);
    if (reverse)
        for (size_t i = 0; i < len; ++i) v[i] = (uint8_t)(3 - base_bit((unsigned char)buf[len - i - 1]));
    else
        for (size_t i = 0; i < len; ++i) v[i] = base_bit((unsigned char)buf[i]);
}

struct Group {
    std::vector<int> ids;
    size_t sum_len = 0;
};

// main.c:124-129
inline bool len_in_group(const Group &g, uint32_t len, int tol)
{
    size_t tmp = (size_t)len * g.ids.size();
    size_t diff = tmp > g.sum_len ? tmp - g.sum_len : g.sum_len - tmp;
    return diff * 100 < (size_t)tol * g.sum_len;
}

// main.c:131-137
inline bool group_in_group(const Group &g, const Group &q, int tol)
{
    size_t a = g.sum_len * q.ids.size(), b = q.sum_len * g.ids.size();
    size_t diff = a > b ? a - b : b - a;
    return diff * 100 < a * (size_t)tol;
}

// main.c:139-212.  bubble_sort_array's tie order is unknown offline (bsalign
// un-vendored): groups are stably sorted by size, largest first (SPEC.md §8).
std::vector<Group> init_group_lens(const uint32_t *a, int n, int tol)
{
    std::vector<Group> g(n);
    for (int i = 0; i < n; ++i) {
        int j;
        for (j = 0; j < i; ++j) {
            if (!g[j].sum_len) continue;
            if (len_in_group(g[j], a[i], tol)) {
                g[j].ids.push_back(i);
                g[j].sum_len += a[i];
                break;
            }
        }
        if (j < i) continue;
        g[j].ids.push_back(i);
        g[j].sum_len = a[i];
    }
    for (bool flag = true; flag;) {
        flag = false;
        for (int j = 0; j < n; ++j) {
            if (g[j].ids.empty()) continue;
            for (int k = 0; k < j; ++k) {
                if (!g[k].ids.empty() && group_in_group(g[k], g[j], tol)) {
                    g[k].ids.insert(g[k].ids.end(), g[j].ids.begin(), g[j].ids.end());
                    g[k].sum_len += g[j].sum_len;
                    g[j].ids.clear();
                    g[j].sum_len = 0;
                    flag = true;
                    break;
                }
            }
        }
    }
    std::vector<Group> out;
    for (auto &x : g)
        if (!x.ids.empty()) out.push_back(std::move(x));
    std::stable_sort(out.begin(), out.end(), [](const Group &x, const Group &y) { return x.ids.size() > y.ids.size(); });
    return out;
}

// main.c:255-290: strand_match's acceptance test on an alignment of q to t
inline bool strand_accept(const ccsx_pairaln &r, uint32_t qlen_, uint32_t tlen_, int sim)
{
    const int qlen = (int)qlen_, tlen = (int)tlen_;
    return r.aln * 2 > (qlen > tlen ? tlen : qlen) && r.mat * 100 >= r.aln * sim;
}

struct Seg {
    uint32_t offs, len;
    uint8_t reverse;
};

}  // namespace

// ccs_prepare (main.c:300-453) as a resumable walk: it runs until a decision
// needs strand_match, hands out both alignments of that decision as one
// request, and goes on when they are answered.  Phase 0 is get_template_grp
// (main.c:300-342: per candidate group the head and the tail check), phases 1
// and 2 the walk from the template towards the first and the last subread
// (main.c:344-453: per abnormal subread the forward and the reverse template).
struct ccsx_prep {
    const char *seqs;
    const uint32_t *lens;
    uint32_t n;
    std::vector<uint32_t> offs, map_group;
    std::vector<Group> groups;
    uint32_t tg = 0, cg = 1, ti = 0, toffs = 0, tlen = 0;
    std::vector<Seg> segs;
    std::vector<uint8_t> tseq, t2seq, qseq, border[2], main_seq[2];
    bool have_t = false;
    int phase = 0;  // 3 = finished
    int64_t k = 0;  // the subread the walk is at
    uint8_t reverse = 0;
    bool strand_adjust = false;
    Seg cur{0, 0, 0};
    uint32_t npend = 0, unused = 0;
    ccsx_pair want[2];

    static constexpr int tol = 10;

    void ask(const std::vector<uint8_t> &q0, const std::vector<uint8_t> &t0, const std::vector<uint8_t> &q1,
             const std::vector<uint8_t> &t1)
    {
        want[0] = ccsx_pair{q0.data(), (uint32_t)q0.size(), t0.data(), (uint32_t)t0.size()};
        want[1] = ccsx_pair{q1.data(), (uint32_t)q1.size(), t1.data(), (uint32_t)t1.size()};
        npend = 2;
    }

    // main.c:300-342 up to the next candidate group's checks; false: asked
    bool template_step()
    {
        if (groups[0].ids.size() < 2) return true;
        for (; cg < groups.size(); ++cg) {
            if (groups[cg].ids.size() < 2 || groups[cg].ids.size() * 5 < 4 * groups[0].ids.size()) continue;
            const uint32_t ci = (uint32_t)groups[cg].ids[groups[cg].ids.size() / 2];
            const uint32_t clen = lens[ci];
            if (clen <= lens[groups[tg].ids[groups[tg].ids.size() / 2]] || clen <= 2000) continue;
            recap(border[0], seqs + offs[ci], 1000, true);
            recap(main_seq[0], seqs + offs[ci] + 1000, clen - 1000, false);
            recap(border[1], seqs + offs[ci] + clen - 1000, 1000, true);
            recap(main_seq[1], seqs + offs[ci], clen - 1000, false);
            ask(border[0], main_seq[0], border[1], main_seq[1]);
            return false;
        }
        return true;
    }

    // one subread of the walk (the body of main.c:370-450's loops); false: asked
    bool visit()
    {
        reverse = reverse == 0 ? 1 : 0;
        cur = Seg{offs[k], lens[k], reverse};
        if (map_group[k] != tg) {
            strand_adjust = true;
            if (cur.len < tlen) return true;
        } else if (!strand_adjust) {
            segs.push_back(cur);
            return true;
        }
        if (!have_t) {
            recap(tseq, seqs + toffs, tlen, false);
            recap(t2seq, seqs + toffs, tlen, true);
            have_t = true;
        }
        recap(qseq, seqs + cur.offs, cur.len, false);
        ask(qseq, tseq, qseq, t2seq);
        return false;
    }

    void advance()
    {
        for (;;) {
            if (phase == 0) {
                if (!template_step()) return;
                ti = (uint32_t)groups[tg].ids[groups[tg].ids.size() / 2];
                toffs = offs[ti], tlen = lens[ti];
                segs.push_back(Seg{toffs, tlen, 0});
                phase = 1, k = (int64_t)ti - 1, reverse = 0, strand_adjust = false;
            } else if (phase == 1) {
                if (k < 0) {
                    phase = 2, k = (int64_t)ti + 1, reverse = 0, strand_adjust = false;
                    continue;
                }
                if (!visit()) return;
                --k;
            } else if (phase == 2) {
                if (k >= (int64_t)n) {
                    phase = 3;
                    return;
                }
                if (!visit()) return;
                ++k;
            } else {
                return;
            }
        }
    }

    void answer(const ccsx_pairaln res[2])
    {
        const bool ok0 = strand_accept(res[0], want[0].qlen, want[0].tlen, phase == 0 ? 70 : 75);
        const bool ok1 = !ok0 && strand_accept(res[1], want[1].qlen, want[1].tlen, phase == 0 ? 70 : 75);
        unused += ok0;
        npend = 0;
        if (phase == 0) {
            if (!ok0 && !ok1) tg = cg;
            ++cg;
        } else {
            if (ok0 || ok1) {
                const ccsx_pairaln &rs = res[ok0 ? 0 : 1];
                reverse = ok0 ? 0 : 1;
                cur.offs += rs.qb, cur.len = rs.qe - rs.qb, cur.reverse = reverse;
                if (len_in_group(groups[tg], cur.len, tol)) segs.push_back(cur);
                strand_adjust = map_group[k] != tg;
            } else {
                strand_adjust = true;
            }
            k += phase == 1 ? -1 : 1;
        }
        advance();
    }
};

extern "C" {

void ccsx_revcomp(char *s, uint32_t l)
{
    unsigned char *seq = reinterpret_cast<unsigned char *>(s);
    for (uint32_t i = 0; i < l >> 1; ++i) {
        unsigned char t = seq[l - 1 - i];
        seq[l - i - 1] = kComp.t[seq[i]];
        seq[i] = kComp.t[t];
    }
    if (l & 1) seq[l >> 1] = kComp.t[seq[l >> 1]];
}

ccsx_prep *ccsx_prep_begin(const char *seqs, const uint32_t *lens, uint32_t n)
{
    ccsx_prep *p = new ccsx_prep;
    p->seqs = seqs, p->lens = lens, p->n = n;
    if (n == 0) {
        p->phase = 3;
        return p;
    }
    p->offs.resize(n);
    for (uint32_t i = 0, o = 0; i < n; o += lens[i], ++i) p->offs[i] = o;
    p->groups = init_group_lens(lens, (int)n, ccsx_prep::tol);
    p->map_group.resize(n);
    for (uint32_t i = 0; i < p->groups.size(); ++i)
        for (int id : p->groups[i].ids) p->map_group[id] = i;
    p->advance();
    return p;
}

uint32_t ccsx_prep_pending(ccsx_prep *p, ccsx_pair want[2])
{
    if (!p->npend) return 0;
    want[0] = p->want[0], want[1] = p->want[1];
    return p->npend;
}

void ccsx_prep_answer(ccsx_prep *p, const ccsx_pairaln res[2])
{
    if (p->npend) p->answer(res);
}

uint32_t ccsx_prep_unused(const ccsx_prep *p) { return p->unused; }

uint32_t ccsx_prep_end(ccsx_prep *p, uint32_t *seg_off, uint32_t *seg_len, uint8_t *seg_rev)
{
    // (a walk ended while a request is pending yields no list)
    const uint32_t ns = p->phase == 3 ? (uint32_t)p->segs.size() : 0;
    for (uint32_t i = 0; i < ns; ++i) {
        if (seg_off) seg_off[i] = p->segs[i].offs;
        if (seg_len) seg_len[i] = p->segs[i].len;
        if (seg_rev) seg_rev[i] = p->segs[i].reverse;
    }
    delete p;
    return ns;
}

// main.c:344-453: the resumable walk with ccsx_pairwise as the answerer
uint32_t ccsx_prepare(const char *seqs, const uint32_t *lens, uint32_t n, uint32_t *seg_off, uint32_t *seg_len,
                      uint8_t *seg_rev)
{
    if (n == 0) return 0;
    ccsx_prep *p = ccsx_prep_begin(seqs, lens, n);
    ccsx_pair w[2];
    while (ccsx_prep_pending(p, w)) {
        ccsx_pairaln r[2];
        memset(r, 0, sizeof r);
        r[0] = ccsx_pairwise(w[0].q, w[0].qlen, w[0].t, w[0].tlen);
        // (strand_match on the second pair only where the first is refused)
        if (!strand_accept(r[0], w[0].qlen, w[0].tlen, p->phase == 0 ? 70 : 75))
            r[1] = ccsx_pairwise(w[1].q, w[1].qlen, w[1].t, w[1].tlen);
        ccsx_prep_answer(p, r);
    }
    return ccsx_prep_end(p, seg_off, seg_len, seg_rev);
}

uint32_t ccsx_prepare_apply(char *seqs, const uint32_t *lens, uint32_t n, uint32_t *seg_off, uint32_t *seg_len)
{
    std::vector<uint8_t> rev(n ? n : 1);
    uint32_t ns = ccsx_prepare(seqs, lens, n, seg_off, seg_len, rev.data());
    for (uint32_t l = 0; l < ns; ++l)
        if (rev[l]) ccsx_revcomp(seqs + seg_off[l], seg_len[l]);
    return ns;
}

}  // extern "C"
