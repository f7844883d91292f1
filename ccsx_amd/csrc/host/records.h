// records.h -- the text of the host program's output files (SPEC.md sections
// 9-17): one formatter per side file over plain arrays, each appending to a
// string.  No FILE, no device context and none of main.cpp's types, so that
// tools/records_sanitize.cpp can drive every formatter on the CPU.  Part of
// the ccsx binary only (not of libccsx_amd.so).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "ccsx_gpu.h"
#include "ccsx_host.h"

namespace ccsx_rec {

// the first line of the -r, -k, -D and -i files
extern const char *const kPassHeader, *const kSamHeader, *const kDemuxHeader, *const kHitHeader;

// a -B barcode set or a -I adapter set: the sequences back to back
struct SeqSet {
    std::vector<std::string> names;
    std::string seqs;
    std::vector<uint32_t> off, len;
    uint32_t size() const { return (uint32_t)len.size(); }
    // the records of a FASTA / FASTQ file (ccsx_barcode_read); false if it
    // cannot be opened or holds none.  The caller checks the set
    // (ccsx_barcode_check / ccsx_scan_check)
    bool read(const char *path);
};

// One FASTA record, or with fastq one FASTQ record: '>' / '@' + header, the n
// bases and, with fastq, "+" and the n qualities (as characters, Q + 33; the
// uint8_t overload takes raw Q)
void append_record(std::string &s, bool fastq, const std::string &header, const char *bases, size_t n, const char *qual);
void append_record(std::string &s, bool fastq, const std::string &header, const char *bases, size_t n, const uint8_t *qual);

// The header of a CCS read in the main output: its name, with fastq followed
// by np= (its passes) and rq= (ccsx_qual_rq of its qualities)
std::string read_header(const std::string &name, bool fastq, size_t np, double rq);

// -r (SPEC.md section 10): one row per segment, from its pass record
void pass_rows(std::string &s, const std::string &name, const ccsx_pass_stat *st, uint32_t nseg, const uint32_t *seg_off,
               const uint32_t *seg_len);

// -a (section 11): the PAF line of segment k of ZMW zmw (movie/hole) from its
// map words; nothing for a map without an aligned base.  Query coordinates on
// the subread's own strand, CIGAR in CCS order
void paf_line(std::string &s, const std::string &zmw, const std::string &name, size_t k, const uint32_t *map, uint32_t len,
              bool rev, uint32_t seg_off, uint32_t ccs_len);

// -s (section 12): one line per position whose two strands call differently
void site_lines(std::string &s, const std::string &name, const ccsx_pileup *pu, uint32_t len, const char *ccs);

// -k (section 13): the read's SAM line; qual (Q + 33) and rq only with fastq,
// nrev of its np segments reverse.  The four arrays only where the ZMW came
// with kinetics (kin != NULL: its len records); returns whether it carries them
bool sam_line(std::string &s, const std::string &name, const char *ccs, uint32_t len, bool fastq, const std::string &qual,
              double rq, size_t np, size_t nrev, const ccsx_kinetics *kin);

// -b (section 14): the record of strand sd (0 forward, 1 reverse) built from
// np segments, laid out as the main output's; nothing for an empty one
void strand_record(std::string &s, bool fastq, const std::string &name, int sd, size_t np, const char *seq,
                   const uint8_t *qual, uint32_t len);

// -p (section 15): the record of the polished read
void polished_record(std::string &s, bool fastq, const std::string &name, const char *seq, const uint8_t *qual, uint32_t len);

// -D (section 16): the read's line of the demultiplexing report
void demux_row(std::string &s, const std::string &name, uint32_t n, const ccsx_bc_out &r, const ccsx_bc_call &call,
               const std::vector<std::string> &names);
// -d: the trimmed record of an assigned read (nothing otherwise): the read's
// own header, then the pair, the two scores and the two clips
void demux_record(std::string &s, bool fastq, const std::string &header, const std::string &ccs, const std::string &qual,
                  const ccsx_bc_out &r, const ccsx_bc_call &call, const std::vector<std::string> &names);

// -i (section 17): one row per hit of a read of n bases
void hit_rows(std::string &s, const std::string &name, uint32_t n, const ccsx_scan_hit *hits, uint64_t nhits,
              const SeqSet &adapters);
// -S: the records of the read's pieces of at least min_piece bases (ccsx_scan_cut)
void piece_records(std::string &s, bool fastq, const std::string &name, const std::string &ccs, const std::string &qual,
                   const ccsx_scan_hit *hits, uint64_t nhits, const SeqSet &adapters, uint32_t min_piece);

// -g (section 18): the PAF line of a reported read of n bases from its record
// and the words of its path; query coordinates on the read as written
void ref_line(std::string &s, const std::string &name, uint32_t n, const ccsx_ref_rec &r, const uint32_t *words,
              const SeqSet &refs);

}  // namespace ccsx_rec
