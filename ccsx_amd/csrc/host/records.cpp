// records.cpp -- the text of the host program's output files (records.h)
#include "records.h"

#include <cstdio>
#include <cstring>

namespace ccsx_rec {

const char *const kPassHeader = "#name\tpass\tsbeg\tslen\tmatch\tmismatch\tins\tdel\tcbeg\tcend\tidentity\n";
const char *const kSamHeader = "@HD\tVN:1.6\tSO:unknown\n";
const char *const kDemuxHeader =
    "#name\tlen\tbc0\tstrand0\tscore0\tsecond0\tend0\tbc1\tstrand1\tscore1\tsecond1\tend1\tcl\tcr\tcalled0\tcalled1\tassigned\treason\n";
const char *const kHitHeader = "#name\tlen\tadapter\tstrand\tstart\tend\tscore\talen\n";

bool SeqSet::read(const char *path)
{
    ccsx_barcode_set *set = ccsx_barcode_read(path);
    const char *const *nm = nullptr, *const *sq = nullptr;
    const uint32_t n = ccsx_barcode_set_get(set, &nm, &sq);
    for (uint32_t k = 0; k < n; ++k) {
        names.push_back(nm[k]);
        off.push_back((uint32_t)seqs.size());
        len.push_back((uint32_t)strlen(sq[k]));
        seqs += sq[k];
    }
    ccsx_barcode_set_free(set);
    return n != 0;
}

namespace {

// '>' / '@' + header, the bases and, with fastq, the "+" line
void record_head(std::string &s, bool fastq, const std::string &header, const char *bases, size_t n)
{
    s += fastq ? '@' : '>';
    s += header;
    s += '\n';
    s.append(bases, n);
    s += '\n';
    if (fastq) s += "+\n";
}

}  // namespace

void append_record(std::string &s, bool fastq, const std::string &header, const char *bases, size_t n, const char *qual)
{
    record_head(s, fastq, header, bases, n);
    if (!fastq) return;
    s.append(qual, n);
    s += '\n';
}

void append_record(std::string &s, bool fastq, const std::string &header, const char *bases, size_t n, const uint8_t *qual)
{
    record_head(s, fastq, header, bases, n);
    if (!fastq) return;
    for (size_t k = 0; k < n; ++k) s += (char)(qual[k] + 33);
    s += '\n';
}

std::string read_header(const std::string &name, bool fastq, size_t np, double rq)
{
    if (!fastq) return name;
    char num[96];
    snprintf(num, sizeof num, " np=%zu rq=%.6f", np, rq);
    return name + num;
}

void pass_rows(std::string &s, const std::string &name, const ccsx_pass_stat *st, uint32_t nseg, const uint32_t *seg_off,
               const uint32_t *seg_len)
{
    char row[192];
    for (uint32_t k = 0; k < nseg; ++k) {
        const ccsx_pass_stat &p = st[k];
        snprintf(row, sizeof row, "\t%zu\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%.6f\n", (size_t)k, seg_off[k], seg_len[k], p.match,
                 p.mismatch, p.ins, p.del, p.cbeg, p.cend, ccsx_pass_identity(&p));
        s += name;
        s += row;
    }
}

void paf_line(std::string &s, const std::string &zmw, const std::string &name, size_t k, const uint32_t *map, uint32_t len,
              bool rev, uint32_t seg_off, uint32_t ccs_len)
{
    ccsx_map_aln a;
    const long n = ccsx_map_cigar(map, len, &a, nullptr, 0);
    if (n < 0) return;
    char head[160];
    snprintf(head, sizeof head, "/%zu\t%u\t%u\t%u\t%c\t", k, len, rev ? len - a.qe : a.qs, rev ? len - a.qs : a.qe,
             rev ? '-' : '+');
    s += zmw;
    s += head;
    s += name;
    snprintf(head, sizeof head, "\t%u\t%u\t%u\t%u\t%u\t255\tsb:i:%u\tcg:Z:", ccs_len, a.ts, a.te, a.n_eq,
             a.n_eq + a.n_x + a.n_ins + a.n_del, seg_off);
    s += head;
    const size_t at = s.size();
    s.resize(at + (size_t)n + 1);
    (void)ccsx_map_cigar(map, len, &a, &s[at], (size_t)n + 1);
    s.resize(at + (size_t)n);
    s += '\n';
}

void site_lines(std::string &s, const std::string &name, const ccsx_pileup *pu, uint32_t len, const char *ccs)
{
    char line[160];
    for (uint32_t p = 0; p < len; ++p) {
        const int cf = ccsx_pileup_call(&pu[p], 0), cr = ccsx_pileup_call(&pu[p], 1);
        if (cf < 0 || cr < 0 || cf == cr) continue;
        const uint8_t *a = pu[p].fwd, *b = pu[p].rev;
        snprintf(line, sizeof line, "\t%u\t%c\t%c\t%c\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\n", p, ccs[p], "ACGT-"[cf],
                 "ACGT-"[cr], a[0], a[1], a[2], a[3], a[4], a[5], b[0], b[1], b[2], b[3], b[4], b[5]);
        s += name;
        s += line;
    }
}

bool sam_line(std::string &s, const std::string &name, const char *ccs, uint32_t len, bool fastq, const std::string &qual,
              double rq, size_t np, size_t nrev, const ccsx_kinetics *kin)
{
    char num[96];
    s += name;
    s += "\t4\t*\t0\t255\t*\t*\t0\t0\t";
    s.append(ccs, len);
    s += '\t';
    if (fastq) s += qual;
    else s += '*';
    snprintf(num, sizeof num, "\tnp:i:%zu", np);
    s += num;
    if (fastq) {
        snprintf(num, sizeof num, "\trq:f:%.6f", rq);
        s += num;
    }
    snprintf(num, sizeof num, "\tfn:i:%zu\trn:i:%zu", np - nrev, nrev);
    s += num;
    if (kin) {
        const long n = ccsx_kinetics_tags(kin, len, nullptr, 0);
        const size_t at = s.size() + 1;
        s += '\t';
        s.resize(at + (size_t)n + 1);
        (void)ccsx_kinetics_tags(kin, len, &s[at], (size_t)n + 1);
        s.resize(at + (size_t)n);
    }
    s += '\n';
    return kin != nullptr;
}

void strand_record(std::string &s, bool fastq, const std::string &name, int sd, size_t np, const char *seq,
                   const uint8_t *qual, uint32_t len)
{
    if (!len) return;
    append_record(s, fastq, read_header(name + (sd ? "/rev" : "/fwd"), fastq, np, fastq ? ccsx_qual_rq(qual, len) : 0), seq,
                  len, qual);
}

void polished_record(std::string &s, bool fastq, const std::string &name, const char *seq, const uint8_t *qual, uint32_t len)
{
    append_record(s, fastq, name + "/polished", seq, len, qual);
}

void demux_row(std::string &s, const std::string &name, uint32_t n, const ccsx_bc_out &r, const ccsx_bc_call &call,
               const std::vector<std::string> &names)
{
    static const char *const why[] = {"ok", "end0", "end1", "ends", "insert"};
    char num[160];
    snprintf(num, sizeof num, "\t%u", n);
    s += name;
    s += num;
    for (int k = 0; k < 2; ++k) {
        const ccsx_bc_end &e = r.e[k];
        s += '\t';
        s += names[(size_t)e.pattern >> 1];
        const char o = (e.pattern & 1) ? '-' : '+';
        // (the runner-up's score: "." for a set of one barcode, which has none)
        if (e.second_pattern < 0) snprintf(num, sizeof num, "\t%c\t%d\t.\t%d", o, e.score, e.end);
        else snprintf(num, sizeof num, "\t%c\t%d\t%d\t%d", o, e.score, e.second, e.end);
        s += num;
    }
    snprintf(num, sizeof num, "\t%u\t%u\t%d\t%d\t%d\t%s\n", call.cl, call.cr, call.called[0], call.called[1], call.assigned,
             why[call.reason]);
    s += num;
}

void demux_record(std::string &s, bool fastq, const std::string &header, const std::string &ccs, const std::string &qual,
                  const ccsx_bc_out &r, const ccsx_bc_call &call, const std::vector<std::string> &names)
{
    if (!call.assigned) return;
    char num[160];
    snprintf(num, sizeof num, " bs=%d,%d bx=%u,%u", r.e[0].score, r.e[1].score, call.cl, call.cr);
    const size_t n = ccs.size() - call.cl - call.cr;
    append_record(s, fastq, header + " bc=" + names[(size_t)r.e[0].pattern >> 1] + "--" + names[(size_t)r.e[1].pattern >> 1] + num,
                  ccs.data() + call.cl, n, qual.data() + (fastq ? call.cl : 0));
}

void hit_rows(std::string &s, const std::string &name, uint32_t n, const ccsx_scan_hit *hits, uint64_t nhits,
              const SeqSet &adapters)
{
    char num[160];
    for (uint64_t k = 0; k < nhits; ++k) {
        const ccsx_scan_hit &h = hits[k];
        snprintf(num, sizeof num, "\t%c\t%u\t%u\t%d\t%u\n", h.orient ? '-' : '+', h.start, h.end, h.score, adapters.len[h.adapter]);
        s += name + '\t' + std::to_string(n) + '\t' + adapters.names[h.adapter] + num;
    }
}

void piece_records(std::string &s, bool fastq, const std::string &name, const std::string &ccs, const std::string &qual,
                   const ccsx_scan_hit *hits, uint64_t nhits, const SeqSet &adapters, uint32_t min_piece)
{
    const uint32_t n = (uint32_t)ccs.size();
    std::vector<ccsx_scan_piece> pcs((size_t)ccsx_scan_cut(hits, nhits, n, min_piece, nullptr, 0));
    ccsx_scan_cut(hits, nhits, n, min_piece, pcs.data(), pcs.size());
    // the flanking hit's adapter and orientation; "." at a read's end
    auto flank = [&](int32_t k) {
        return k < 0 ? std::string(".") : adapters.names[hits[k].adapter] + (hits[k].orient ? '-' : '+');
    };
    char num[64];
    for (const ccsx_scan_piece &p : pcs) {
        snprintf(num, sizeof num, "/%u_%u", p.b, p.e);
        append_record(s, fastq, name + num + " la=" + flank(p.left) + " ra=" + flank(p.right), ccs.data() + p.b, p.e - p.b,
                      qual.data() + (fastq ? p.b : 0));
    }
}

void ref_line(std::string &s, const std::string &name, uint32_t n, const ccsx_ref_rec &r, const uint32_t *words,
              const SeqSet &refs)
{
    ccsx_map_aln a;
    const long c = ccsx_map_cigar(words, n, &a, nullptr, 0);
    if (c < 0 || r.g < 0) return;
    const uint32_t qb = (uint32_t)r.a.qb, qe = (uint32_t)r.a.qe;
    char num[256];
    snprintf(num, sizeof num, "\t%u\t%u\t%u\t%c\t", n, r.o ? n - qe : qb, r.o ? n - qb : qe, r.o ? '-' : '+');
    s += name + num + refs.names[(size_t)r.g];
    snprintf(num, sizeof num, "\t%u\t%d\t%d\t%d\t%d\t255\tAS:i:%d\tsv:i:%d\ts2:i:%d\tcg:Z:", refs.len[(size_t)r.g], r.a.tb, r.a.te,
             r.a.mat, r.a.aln, r.a.score, r.votes, r.votes2);
    s += num;
    const size_t at = s.size();
    s.resize(at + (size_t)c + 1);
    (void)ccsx_map_cigar(words, n, &a, &s[at], (size_t)c + 1);
    s.resize(at + (size_t)c);
    s += '\n';
}

}  // namespace ccsx_rec
