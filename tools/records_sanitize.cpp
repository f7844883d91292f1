// records_sanitize.cpp -- drives the host program's record formatters
// (ccsx_amd/csrc/host/records.h) under AddressSanitizer +
// UndefinedBehaviorSanitizer on the CPU.  tests/test_records_host.py compiles it
// with records.cpp and the host sources the formatters call (no HIP code).
//
//   records_sanitize
//     every formatter on small constructed inputs, the edges its code branches
//     on among them, each text compared with the one written out here; prints
//     "ok <checks>"
//   records_sanitize <reads.fa|fq> <barcodes.fa> <adapters.fa> <out prefix>
//     the -d / -D / -i / -S texts of the reads (records of two lines, or of
//     four with qualities; a read's header as the main output writes it) by
//     ccsx_barcode_host + ccsx_barcode_call and ccsx_scan_host + ccsx_scan_cut
//     at the program's defaults (-W 96 -T 60 -L 3 -E 75 -e 50), written to
//     <out prefix>.d / .D / .i / .S; prints "ok <reads>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "records.h"

using namespace ccsx_rec;

static int checks = 0, failed = 0;

static void expect(const std::string &got, const std::string &want, const char *what)
{
    ++checks;
    if (got == want) return;
    ++failed;
    fprintf(stderr, "records_sanitize: %s\n  got  [%s]\n  want [%s]\n", what, got.c_str(), want.c_str());
}

// a string's bytes in a buffer of exactly its length (no NUL follows)
static std::vector<char> exact(const std::string &s) { return std::vector<char>(s.begin(), s.end()); }

static int constructed()
{
    const std::string name = "mv/7/ccs";
    std::string s;

    // records: FASTA, FASTQ from characters and from raw qualities; an empty read
    const std::vector<char> acgt = exact("ACGT"), iiii = exact("IIJK");
    const std::vector<uint8_t> raw = {0, 1, 60, 93};
    append_record(s, false, name, acgt.data(), 4, (const char *)nullptr);
    append_record(s, true, name + " x", acgt.data(), 4, iiii.data());
    append_record(s, true, name, acgt.data(), 4, raw.data());
    append_record(s, true, name, acgt.data(), 0, raw.data());
    expect(s, ">mv/7/ccs\nACGT\n@mv/7/ccs x\nACGT\n+\nIIJK\n@mv/7/ccs\nACGT\n+\n!\"]~\n@mv/7/ccs\n\n+\n\n", "append_record");
    expect(read_header(name, false, 3, .5), "mv/7/ccs", "read_header without -q");
    expect(read_header(name, true, 3, .5), "mv/7/ccs np=3 rq=0.500000", "read_header with -q");

    // -r: two segments, the second one's record empty (identity 0)
    const std::vector<ccsx_pass_stat> st = {{9, 1, 0, 0, 2, 12}, {0, 0, 0, 0, 0, 0}};
    const std::vector<uint32_t> so = {0, 40}, sl = {10, 7};
    s.clear();
    pass_rows(s, name, st.data(), 2, so.data(), sl.data());
    expect(s, "mv/7/ccs\t0\t0\t10\t9\t1\t0\t0\t2\t12\t0.900000\nmv/7/ccs\t1\t40\t7\t0\t0\t0\t0\t0\t0\t0.000000\n", "pass_rows");
    s.clear();
    pass_rows(s, name, nullptr, 0, nullptr, nullptr);
    expect(s, "", "pass_rows of no segment");

    // -a: a forward segment, a reverse one whose first base is an insertion, and a map without an aligned base
    const std::vector<uint32_t> fwd = {0, 1, 2 | CCSX_MAP_MISMATCH, 3 | CCSX_MAP_INS, 3};
    const std::vector<uint32_t> rev = {0 | CCSX_MAP_INS, 0, 1, 4};
    const std::vector<uint32_t> none = {2 | CCSX_MAP_INS, 2 | CCSX_MAP_INS};
    s.clear();
    paf_line(s, "mv/7", name, 0, fwd.data(), 5, false, 0, 10);
    paf_line(s, "mv/7", name, 1, none.data(), 2, false, 5, 10);
    paf_line(s, "mv/7", name, 2, rev.data(), 4, true, 7, 10);
    paf_line(s, "mv/7", name, 3, nullptr, 0, true, 11, 10);
    expect(s,
           "mv/7/0\t5\t0\t5\t+\tmv/7/ccs\t10\t0\t4\t3\t5\t255\tsb:i:0\tcg:Z:2=1X1I1=\n"
           "mv/7/2\t4\t0\t3\t-\tmv/7/ccs\t10\t0\t5\t3\t5\t255\tsb:i:7\tcg:Z:2=2D1=\n",
           "paf_line");

    // -s: a concordant position, one with an empty strand, a discordant base / base and a base / gap one
    const std::vector<ccsx_pileup> pu = {{{5, 0, 0, 0, 0, 1}, {4, 0, 0, 0, 0, 0}},
                                         {{0, 0, 0, 0, 0, 0}, {0, 3, 0, 0, 0, 0}},
                                         {{5, 0, 0, 0, 0, 1}, {0, 4, 0, 0, 0, 0}},
                                         {{0, 0, 0, 6, 1, 0}, {0, 0, 0, 2, 3, 2}}};
    const std::vector<char> ccs4 = exact("AAAT");
    s.clear();
    site_lines(s, name, pu.data(), 2, ccs4.data());
    expect(s, "", "site_lines without a discordant site");
    site_lines(s, name, pu.data(), 4, ccs4.data());
    expect(s, "mv/7/ccs\t2\tA\tA\tC\t5\t0\t0\t0\t0\t1\t0\t4\t0\t0\t0\t0\nmv/7/ccs\t3\tT\tT\t-\t0\t0\t0\t6\t1\t0\t0\t0\t0\t2\t3\t2\n",
           "site_lines");

    // -k: with and without -q, with and without the arrays
    const std::vector<ccsx_kinetics> kin = {{{10, 20, 2}, {11, 21, 1}, {0, 0}}, {{12, 22, 2}, {0, 0, 0}, {0, 0}},
                                            {{13, 23, 2}, {14, 24, 1}, {0, 0}}, {{15, 25, 2}, {16, 26, 1}, {0, 0}}};
    const std::string plain = "mv/7/ccs\t4\t*\t0\t255\t*\t*\t0\t0\tACGT\t*\tnp:i:5\tfn:i:3\trn:i:2";
    const std::string withq = "mv/7/ccs\t4\t*\t0\t255\t*\t*\t0\t0\tACGT\tIIJK\tnp:i:5\trq:f:0.990000\tfn:i:3\trn:i:2";
    s.clear();
    bool arrays = sam_line(s, name, acgt.data(), 4, false, "", 0, 5, 2, nullptr);
    expect(s, plain + "\n", "sam_line without -q and arrays");
    expect(arrays ? "arrays" : "none", "none", "sam_line's flag without arrays");
    s.clear();
    arrays = sam_line(s, name, acgt.data(), 4, true, "IIJK", .99, 5, 2, nullptr);
    expect(s, withq + "\n", "sam_line with -q, without arrays");
    for (int fastq = 0; fastq < 2; ++fastq) {
        s.clear();
        arrays = sam_line(s, name, acgt.data(), 4, fastq != 0, fastq ? "IIJK" : "", .99, 5, 2, kin.data());
        std::string tags((size_t)ccsx_kinetics_tags(kin.data(), 4, nullptr, 0) + 1, '\0');
        ccsx_kinetics_tags(kin.data(), 4, &tags[0], tags.size());
        tags.pop_back();
        expect(s, (fastq ? withq : plain) + "\t" + tags + "\n", "sam_line with arrays");
        expect(arrays && tags.compare(0, 7, "fi:B:C,") == 0 ? "arrays" : "none", "arrays", "sam_line's flag with arrays");
    }

    // -b: a strand without a base, the forward and the reverse record
    s.clear();
    strand_record(s, true, name, 0, 3, nullptr, nullptr, 0);
    strand_record(s, false, name, 1, 2, nullptr, nullptr, 0);
    expect(s, "", "strand_record of an empty strand");
    const std::vector<uint8_t> q10 = {10, 10, 10, 10};
    strand_record(s, false, name, 0, 3, acgt.data(), nullptr, 4);
    strand_record(s, true, name, 1, 2, acgt.data(), q10.data(), 4);
    expect(s, ">mv/7/ccs/fwd\nACGT\n@mv/7/ccs/rev np=2 rq=0.900000\nACGT\n+\n++++\n", "strand_record");

    // -p
    s.clear();
    polished_record(s, false, name, acgt.data(), nullptr, 4);
    polished_record(s, true, name, acgt.data(), q10.data(), 4);
    expect(s, ">mv/7/ccs/polished\nACGT\n@mv/7/ccs/polished\nACGT\n+\n++++\n", "polished_record");

    // -D / -d: a set of one barcode (no runner-up), assigned; a set of two, one end not called
    const std::vector<std::string> one = {"solo"}, two = {"bcA", "bcB"};
    const std::vector<uint32_t> len16 = {16, 16};
    const std::string read = "AACCGGTTACGTACGTTTGGCCAA", rq = std::string(24, 'I');
    ccsx_bc_out r1 = {{{0, 16, 4, CCSX_BC_NONE, -1}, {1, 14, 5, CCSX_BC_NONE, -1}}};
    ccsx_bc_call call;
    ccsx_barcode_call(&r1, len16.data(), 1, 24, 60, 3, &call);
    std::string row, rec;
    demux_row(row, name, 24, r1, call, one);
    expect(row, "mv/7/ccs\t24\tsolo\t+\t16\t.\t4\tsolo\t-\t14\t.\t5\t4\t5\t1\t1\t1\tok\n", "demux_row of a one-barcode set");
    demux_record(rec, false, name, read, "", r1, call, one);
    demux_record(rec, true, read_header(name, true, 5, .99), read, rq, r1, call, one);
    expect(rec,
           ">mv/7/ccs bc=solo--solo bs=16,14 bx=4,5\nGGTTACGTACGTTTG\n"
           "@mv/7/ccs np=5 rq=0.990000 bc=solo--solo bs=16,14 bx=4,5\nGGTTACGTACGTTTG\n+\nIIIIIIIIIIIIIII\n",
           "demux_record");
    ccsx_bc_out r2 = {{{2, 15, 16, 3, 1}, {1, 4, 7, 3, 2}}};
    ccsx_barcode_call(&r2, len16.data(), 2, 24, 60, 3, &call);
    row.clear(), rec.clear();
    demux_row(row, name, 24, r2, call, two);
    expect(row, "mv/7/ccs\t24\tbcB\t+\t15\t3\t16\tbcA\t-\t4\t3\t7\t16\t0\t1\t0\t0\tend1\n", "demux_row of an unassigned read");
    demux_record(rec, true, name, read, rq, r2, call, two);
    expect(rec, "", "demux_record of an unassigned read");

    // -i / -S: no hit (one piece, no flank); two hits that leave a piece below -e, one between them and one after
    SeqSet ads;
    ads.names = {"ad0", "ad1"}, ads.seqs = "ACGTACGTTTTTT", ads.off = {0, 8}, ads.len = {8, 5};
    s.clear();
    hit_rows(s, name, 24, nullptr, 0, ads);
    expect(s, "", "hit_rows of a read without a hit");
    piece_records(s, false, name, read, "", nullptr, 0, ads, 50);  // (whole, whatever -e says)
    expect(s, ">mv/7/ccs/0_24 la=. ra=.\n" + read + "\n", "piece_records of a read without a hit");
    const std::vector<ccsx_scan_hit> hits = {{0, 1, 1, 2, 7, 5}, {0, 0, 0, 12, 20, 7}};
    s.clear();
    hit_rows(s, name, 24, hits.data(), 2, ads);
    expect(s, "mv/7/ccs\t24\tad1\t-\t2\t7\t5\t5\nmv/7/ccs\t24\tad0\t+\t12\t20\t7\t8\n", "hit_rows");
    s.clear();
    piece_records(s, true, name, read, rq, hits.data(), 2, ads, 3);
    expect(s, "@mv/7/ccs/7_12 la=ad1- ra=ad0+\nTACGT\n+\nIIIII\n@mv/7/ccs/20_24 la=ad0+ ra=.\nCCAA\n+\nIIII\n", "piece_records");

    // the headers end their line
    for (const char *h : {kPassHeader, kSamHeader, kDemuxHeader, kHitHeader})
        expect(std::string(1, h[strlen(h) - 1]), "\n", "a header's last character");
    if (failed) return 1;
    printf("ok %d\n", checks);
    return 0;
}

static int files(const char *reads, const char *bc_path, const char *ad_path, const std::string &prefix)
{
    SeqSet bcs, ads;
    if (!bcs.read(bc_path) || ccsx_barcode_check(bcs.seqs.data(), bcs.off.data(), bcs.len.data(), bcs.size()) != 0 ||
        !ads.read(ad_path) || ccsx_scan_check(ads.seqs.data(), ads.off.data(), ads.len.data(), ads.size(), 75) != 0) {
        fprintf(stderr, "records_sanitize: bad barcode or adapter file\n");
        return 1;
    }
    std::ifstream in(reads);
    std::string text[4] = {"", kDemuxHeader, kHitHeader, ""};  // .d .D .i .S
    std::string head, seq, plus, qual;
    int n = 0;
    while (std::getline(in, head) && std::getline(in, seq)) {
        const bool fastq = head[0] == '@';
        if (fastq && !(std::getline(in, plus) && std::getline(in, qual) && qual.size() == seq.size())) return 1;
        head.erase(0, 1);
        const std::string name = head.substr(0, head.find(' '));
        const std::vector<char> ccs = exact(seq);  // (the stages read exactly its length)
        const uint32_t len = (uint32_t)ccs.size();
        ccsx_bc_out r;
        if (ccsx_barcode_host(bcs.seqs.data(), bcs.off.data(), bcs.len.data(), bcs.size(), 96, ccs.data(), len, &r) != 0) return 1;
        ccsx_bc_call call;
        ccsx_barcode_call(&r, bcs.len.data(), bcs.size(), len, 60, 3, &call);
        demux_record(text[0], fastq, head, seq, qual, r, call, bcs.names);
        demux_row(text[1], name, len, r, call, bcs.names);
        const int64_t nh = ccsx_scan_host(ads.seqs.data(), ads.off.data(), ads.len.data(), ads.size(), 75, ccs.data(), len, nullptr, 0);
        if (nh < 0) return 1;
        std::vector<ccsx_scan_hit> hits((size_t)nh);
        ccsx_scan_host(ads.seqs.data(), ads.off.data(), ads.len.data(), ads.size(), 75, ccs.data(), len, hits.data(), hits.size());
        hit_rows(text[2], name, len, hits.data(), hits.size(), ads);
        piece_records(text[3], fastq, name, seq, qual, hits.data(), hits.size(), ads, 50);
        ++n;
    }
    static const char *const ext[4] = {".d", ".D", ".i", ".S"};
    for (int k = 0; k < 4; ++k) {
        std::ofstream out(prefix + ext[k], std::ios::binary);
        out << text[k];
        if (!out.flush()) return 1;
    }
    printf("ok %d\n", n);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 1) return constructed();
    if (argc == 5) return files(argv[1], argv[2], argv[3], argv[4]);
    fprintf(stderr, "usage: records_sanitize [<reads> <barcodes> <adapters> <out prefix>]\n");
    return 2;
}
