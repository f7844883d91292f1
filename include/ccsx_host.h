/*
 * ccsx_host.h -- the C host program's per-ZMW preparation (CPU side).
 *
 * Restates, for the GPU engine's caller, what ccsx does on its CPU threads
 * before the hot path: ccs_prepare (main.c:344-453: subread length groups,
 * template choice, strand assignment, abnormal-subread re-alignment and
 * trimming) and the in-place strand flip (main.c:471-476 / 527-531, using
 * seq_reverse_comp, seqio.h:138-148).
 */
#ifndef CCSX_HOST_H
#define CCSX_HOST_H
#include <stddef.h>
#include <stdint.h>

#include "ccsx_gpu.h" /* ccsx_zmw_in, ccsx_pairaln, ccsx_aln_ctx */

#ifdef __cplusplus
extern "C" {
#endif

/* seqio.h:120-148 -- in-place reverse complement (IUPAC/lowercase aware). */
void ccsx_revcomp(char *seq, uint32_t len);

/* main.c:344-453.  seqs = the ZMW's subreads concatenated, lens[n] their
 * lengths.  Writes the push list (<= n segments) into seg_off/seg_len/seg_rev
 * and returns its length.  Does not modify seqs. */
uint32_t ccsx_prepare(const char *seqs, const uint32_t *lens, uint32_t n,
                      uint32_t *seg_off, uint32_t *seg_len, uint8_t *seg_rev);

/* ccsx_prepare + the strand flip of every reverse segment, in place in seqs
 * (what ccs_for/ccs_for2 do before the first push). */
uint32_t ccsx_prepare_apply(char *seqs, const uint32_t *lens, uint32_t n,
                            uint32_t *seg_off, uint32_t *seg_len);

/* ccsx_prepare_apply with the ZMW's kinetics planes (SPEC.md section 13): ipd
 * and pw hold one code per base parallel to seqs (either may be NULL); over
 * every reverse segment both are reversed in place, so that base j of the
 * segment as pushed keeps the values of the subread base it came from.
 * seg_rev (may be NULL) receives ccsx_prepare's flags. */
uint32_t ccsx_prepare_apply_kin(char *seqs, uint8_t *ipd, uint8_t *pw, const uint32_t *lens, uint32_t n,
                                uint32_t *seg_off, uint32_t *seg_len, uint8_t *seg_rev);

/* The 8-bit kinetics codec (SPEC.md section 13): byte b stands for
 * ((b & 63) << g) + (64 << g) - 64 frames with g = b >> 6 (0 .. 952);
 * ccsx_kin_code gives the byte whose frames are nearest to min(f, 952), the
 * lower byte on a tie. */
uint32_t ccsx_kin_frames(uint8_t code);
uint8_t ccsx_kin_code(uint32_t frames);

/* The SAM array tags of a ZMW's kinetics records (ccsx_gpu_kinetics; len
 * records): "fi:B:C,..<TAB>fp:B:C,..<TAB>ri:B:C,..<TAB>rp:B:C,.." -- the
 * forward strand's ipd and pw codes in CCS order, the reverse strand's with
 * the last CCS base first.  Returns the length without the NUL, computed even
 * when cap is too small; at most cap bytes are written (NUL-terminated when
 * cap > 0; buf may be NULL with cap 0). */
long ccsx_kinetics_tags(const ccsx_kinetics *rec, uint32_t len, char *buf, size_t cap);

/* The pairwise aligner used by strand_match (main.c:255-290), standing in for
 * bsalign's kmer_striped_seqedit_pairwise(13, ...) (SPEC.md §8).  q/t are
 * 2-bit codes (values >= 4 never match).  Returns aligned columns (aln);
 * ccsx_pairaln is defined in ccsx_gpu.h, beside the device's band aligner. */
ccsx_pairaln ccsx_pairwise(const uint8_t *q, uint32_t qlen, const uint8_t *t, uint32_t tlen);

/* ccsx_pairwise's two halves (SPEC.md §8), so that the band can run elsewhere
 * (ccsx_gpu_band_align, include/ccsx_gpu.h).  ccsx_pairwise_seed: the 13-mer
 * diagonal vote; returns 1 and writes the winning diagonal d0, or 0 when
 * either length is below 13 or no k-mer votes (ccsx_pairwise then gives the
 * all-zero result).  ccsx_pairwise_band: the banded local alignment over the
 * diagonals [d0 - 256, d0 + 256] and its traceback, for any d0 and any
 * lengths.  ccsx_pairwise is their composition. */
int ccsx_pairwise_seed(const uint8_t *q, uint32_t qlen, const uint8_t *t, uint32_t tlen, int32_t *d0);
ccsx_pairaln ccsx_pairwise_band(const uint8_t *q, uint32_t qlen, const uint8_t *t, uint32_t tlen, int32_t d0);

/* ccsx_prepare as a resumable walk, for a caller that answers the alignments
 * of many ZMWs at once (ccsx_prepare_batch).  ccsx_prep_begin starts the walk
 * of one ZMW (seqs and lens must stay valid until ccsx_prep_end) and runs it
 * to its first request.  ccsx_prep_pending copies the open request into want
 * and returns its number of pairs (2), or 0 when the walk has finished.  A
 * request holds both alignments of one decision: for a subread the forward and
 * the reverse template, in get_template_grp the head and the tail check; the
 * second answer is consulted only where strand_match's test, which stays
 * here, refuses the first.  The pairs are 2-bit codes owned by the walk, valid
 * until the next ccsx_prep_answer.  ccsx_prep_answer takes the two results
 * (ccsx_pairwise of each pair, or anything equal to it) and runs on to the
 * next request.  ccsx_prep_unused: the second answers not consulted so far.
 * ccsx_prep_end writes the push list as ccsx_prepare does, returns its length
 * and frees the walk; while a request is pending it writes nothing, returns 0
 * and frees the walk all the same (the arrays may then be NULL).
 * ccsx_prepare is this loop with ccsx_pairwise as the answerer. */
typedef struct {
    const uint8_t *q;
    uint32_t qlen;
    const uint8_t *t;
    uint32_t tlen;
} ccsx_pair;
typedef struct ccsx_prep ccsx_prep;
ccsx_prep *ccsx_prep_begin(const char *seqs, const uint32_t *lens, uint32_t n);
uint32_t ccsx_prep_pending(ccsx_prep *p, ccsx_pair want[2]);
void ccsx_prep_answer(ccsx_prep *p, const ccsx_pairaln res[2]);
uint32_t ccsx_prep_unused(const ccsx_prep *p);
uint32_t ccsx_prep_end(ccsx_prep *p, uint32_t *seg_off, uint32_t *seg_len, uint8_t *seg_rev);

/* ccsx_prepare over nz ZMWs with the band alignments of each round run as one
 * ccsx_gpu_band_align (host/prepare_gpu.cpp): on nthreads threads every walk
 * is begun; per round every wanted pair is seeded on the threads
 * (ccsx_pairwise_seed; a pair without a seed gets the all-zero result and no
 * job), one ccsx_gpu_band_align runs all the jobs, and every walk is answered;
 * until no walk is pending.  ZMW i is seqs[i] / lens[i] / n[i]; its push list
 * goes to seg_off[i] / seg_len[i] / seg_rev[i] (room for n[i] entries each)
 * and its length to nseg[i], all equal to ccsx_prepare's.  info (may be NULL)
 * receives the rounds, the jobs, and the milliseconds spent seeding, in
 * ccsx_gpu_band_align, in its kernels, and in all.  Returns 0, or -1 when the
 * aligner failed (nothing written is valid then; the context's error says
 * why). */
typedef struct {
    uint64_t rounds, jobs;
    double seed_ms, device_ms, kernel_ms, total_ms;
} ccsx_batch_info;
int ccsx_prepare_batch(ccsx_aln_ctx *aln, const char *const *seqs, const uint32_t *const *lens, const uint32_t *n,
                       size_t nz, int nthreads, uint32_t *const *seg_off, uint32_t *const *seg_len,
                       uint8_t *const *seg_rev, uint32_t *nseg, ccsx_batch_info *info);

/* Multi-GPU step 1 of the host program (replaces kt_for's dynamic dealing of
 * ZMW indices over threads, kthread.c:24-46).
 * ccsx_zmw_cost: estimated POA work of one prepared ZMW, S x (28 + nseg) with
 * S = sum of segment lengths.
 * ccsx_partition: nb = min(nparts, n / min_batch) batches (at least one);
 * the ZMWs ranked by decreasing cost (ties in input order) and rank r dealt to
 * batch r % nb, so batch costs differ by at most one ZMW's cost.  Batch b is
 * order[bounds[b] .. bounds[b+1]), in decreasing cost.  bounds needs room for
 * n + 1 entries.  Returns nb. */
uint64_t ccsx_zmw_cost(const uint32_t *seg_len, uint32_t nseg);
uint32_t ccsx_partition(const uint64_t *cost, uint32_t n, uint32_t nparts, uint32_t min_batch,
                        uint32_t *order, uint32_t *bounds);

/* Per-base consensus quality (SPEC.md section 9), the formula the kernel
 * applies per emitted column: clamp(3 x (2 x match - cov), 2, 93) for a column
 * whose consensus base `match` of the `cov` reads spanning it carry.
 * ccsx_qual_rq: the predicted read accuracy 1 - mean(10^(-Q/10)) over a
 * read's quality bytes (raw, not ASCII), in double; 0.0 for len == 0. */
uint8_t ccsx_qual_phred(uint32_t match, uint32_t cov);
double ccsx_qual_rq(const uint8_t *qual, uint32_t len);

/* Identity of one pass against the consensus (SPEC.md section 10), from its
 * record (ccsx_gpu_pass_stats): match / (match + mismatch + ins + del) in
 * double; 0.0 when the record is empty (or st is NULL). */
double ccsx_pass_identity(const ccsx_pass_stat *st);

/* The alignment of one segment to the CCS derived from its map (SPEC.md
 * section 11; map / len from ccsx_gpu_base_map).  Aligned entries are those
 * without CCSX_MAP_INS: qs = the first one's index, qe = one past the last
 * one's, ts = entry qs's offset, te = entry qe-1's offset + 1; insertions
 * before qs and from qe on lie outside the alignment.  The CIGAR walks
 * [qs, qe) in CCS order: 'I' for an insertion; for an aligned entry first 'D'
 * x (offset - previous aligned offset - 1) if positive, then 'X' with
 * CCSX_MAP_MISMATCH, else '='; equal adjacent operations merged, lengths in
 * decimal.  n_eq / n_x / n_ins / n_del count the operations' bases.
 * Returns the CIGAR's length without the NUL, computed even when cap is too
 * small; at most cap bytes are written (NUL-terminated when cap > 0, cut short
 * if it does not fit; cigar may be NULL with cap 0).  Returns -1, *aln zeroed
 * and an empty string, for a map without an aligned entry.  aln may be NULL. */
typedef struct {
    uint32_t qs, qe, ts, te, n_eq, n_x, n_ins, n_del;
} ccsx_map_aln;
long ccsx_map_cigar(const uint32_t *map, uint32_t len, ccsx_map_aln *aln, char *cigar, size_t cap);

/* The call of one strand at a CCS position from its pileup record (SPEC.md
 * section 12; records from ccsx_gpu_pileup): strand 0 = the forward reads'
 * counts, 1 = the reverse reads', 2 = both (the fieldwise sum of the stored
 * bytes).  The column rule on that strand's five counts A, C, G, T, gap: -1 if
 * they sum to 0; else best = the base with the largest count (ties: the
 * smallest), and the call is best (0 .. 3) if its count >= gap, else 4 (gap).
 * A position whose forward and reverse calls are both >= 0 and differ is a
 * discordant site.  -1 also for p == NULL or another strand value. */
int ccsx_pileup_call(const ccsx_pileup *p, int strand);

/* The polish step of one ZMW as a sequential loop (SPEC.md section 15; the
 * device's ccsx_gpu_polish gives the same bytes and runs this for the ZMWs its
 * arena cannot hold).  ccs / len = the draft; seqs, seg_off, seg_len, nseg =
 * the segments as pushed; map = their section 11 words, segments back to back
 * in push order.  Writes the polished read to out_seq / out_qual (capacity
 * 2 len + 1 each; qualities 0..kQMax, not ASCII), the realigned map to out_map
 * (one word per pushed base) and counts[4] = the polished length, nsub, nins,
 * ndel.  Returns 0, or CCSX_POLISH_BAD_MAP (nothing but counts written, all
 * zero) for a map whose offsets decrease within a segment or pass len. */
int32_t ccsx_polish_host(const char *ccs, uint32_t len, const char *seqs, const uint32_t *seg_off,
                         const uint32_t *seg_len, uint32_t nseg, const uint32_t *map, char *out_seq,
                         uint8_t *out_qual, uint32_t *out_map, uint32_t *counts);

/* Barcode demultiplexing of CCS reads (SPEC.md section 16; the device's
 * ccsx_gpu_bc_score gives the same values).
 * ccsx_barcode_check: 0 for a barcode set (1 <= B <= 2048 sequences seqs +
 * off[b] of 1 <= len[b] <= 64 letters ACGT in either case), else -1.
 * ccsx_barcode_host: the definition as a sequential loop, for one read ccs /
 * n (ASCII; n may be 0) and the window length Wn; writes out (ccsx_bc_out,
 * include/ccsx_gpu.h).  Returns 0, or -1 (out untouched) for a bad set or a Wn
 * outside 1 .. 256.
 * ccsx_barcode_call: the call of one read of n bases from its result r: end e
 * is called iff 100 x score >= T x L (L = the length of the winning pattern's
 * barcode, from len) and (B = 1 or score - second >= D); cl / cr = the clip
 * length (r's end) of end 0 / 1 if called, else 0; the read is assigned iff
 * both ends are called and cl + cr < n, and its trimmed read is then
 * ccs[cl, n - cr).  reason: CCSX_BC_OK, or why it is not assigned. */
enum { CCSX_BC_OK = 0, CCSX_BC_NO_END0 = 1, CCSX_BC_NO_END1 = 2, CCSX_BC_NO_ENDS = 3, CCSX_BC_NO_INSERT = 4 };
typedef struct {
    uint32_t cl, cr;
    uint8_t called[2], assigned, reason;
} ccsx_bc_call;
int32_t ccsx_barcode_check(const char *seqs, const uint32_t *off, const uint32_t *len, uint32_t B);
int32_t ccsx_barcode_host(const char *seqs, const uint32_t *off, const uint32_t *len, uint32_t B, uint32_t Wn,
                          const char *ccs, uint32_t n, ccsx_bc_out *out);
void ccsx_barcode_call(const ccsx_bc_out *r, const uint32_t *len, uint32_t B, uint32_t n, int32_t T, int32_t D,
                       ccsx_bc_call *call);
/* A barcode FASTA (or FASTQ; gzip allowed), read with the subread reader's
 * record parser: a record's name is its header up to the first white space.
 * ccsx_barcode_read returns NULL if the file cannot be opened or holds no
 * record; the set is then checked with ccsx_barcode_set_get + ccsx_barcode_check.
 * ccsx_barcode_set_get: the number of records; names / seqs (each may be
 * NULL) receive arrays of that many NUL-terminated strings, owned by the set. */
typedef struct ccsx_barcode_set ccsx_barcode_set;
ccsx_barcode_set *ccsx_barcode_read(const char *path);
uint32_t ccsx_barcode_set_get(const ccsx_barcode_set *s, const char *const **names, const char *const **seqs);
void ccsx_barcode_set_free(ccsx_barcode_set *s);

/* Adapter scan of whole CCS reads (SPEC.md section 17; the device's
 * ccsx_gpu_scan gives the same hits).  An adapter file is read with
 * ccsx_barcode_read.
 * ccsx_scan_check: 0 for an adapter set (1 <= A <= 64 sequences seqs + off[a]
 * of 1 <= len[a] <= 64 letters ACGT in either case) and a threshold
 * 1 <= T <= 100, else -1.
 * ccsx_scan_host: the definition as a sequential loop over one column per
 * pattern, for one read ccs / n (ASCII; n may be 0).  Returns the number of
 * hits and writes the first min(that, cap) of them to hits (may be NULL), by
 * (end, adapter), read = 0: a first call counts, a second fills.  -1 (nothing
 * written) for a bad set or T.
 * ccsx_scan_start: the start of a hit of adapter / L in orientation orient that
 * ends at column end of ccs / n: end - k*, k* the smallest k in
 * [0, min(end, 2 L)] that maximises the anchored G(L, k); score (may be NULL)
 * receives that maximum.  -1 for L outside 1 .. 64 or end > n.
 * ccsx_scan_cut: the pieces of a read of n bases outside the union of its hits
 * (nhits of them, as ccsx_scan_host lists them) that have at least Lmin bases,
 * by b; left / right = the index of the flanking hit, -1 at the read's end.
 * Returns their number and writes the first min(that, cap) to pieces (may be
 * NULL).  A read without a hit is the one piece [0, n). */
typedef struct {
    uint32_t b, e;
    int32_t left, right;
} ccsx_scan_piece;
int32_t ccsx_scan_check(const char *seqs, const uint32_t *off, const uint32_t *len, uint32_t A, uint32_t T);
int64_t ccsx_scan_host(const char *seqs, const uint32_t *off, const uint32_t *len, uint32_t A, uint32_t T, const char *ccs,
                       uint32_t n, ccsx_scan_hit *hits, uint64_t cap);
int32_t ccsx_scan_start(const char *adapter, uint32_t L, uint32_t orient, const char *ccs, uint32_t n, uint32_t end,
                        int32_t *score);
int64_t ccsx_scan_cut(const ccsx_scan_hit *hits, uint64_t nhits, uint32_t n, uint32_t Lmin, ccsx_scan_piece *pieces,
                      uint64_t cap);

/* Mapping of CCS reads to a reference set (SPEC.md section 18; the device's
 * ccsx_gpu_ref_map gives the same records and words).  A reference file is
 * read with ccsx_barcode_read.
 * ccsx_pairwise_band_path: ccsx_pairwise_band that also writes the path: one
 * section 11 word per query base into words[qlen] (may be NULL): the target
 * offset of an aligned base (CCSX_MAP_MISMATCH if the bases differ),
 * CCSX_MAP_INS | the offset it is inserted before; CCSX_MAP_INS | tb before qb
 * and CCSX_MAP_INS | te from qe on (CCSX_MAP_INS | 0 throughout for the
 * all-zero result).
 * ccsx_ref_set_make: the checked and coded set with its index, or NULL if it
 * is not one: 1 <= G <= 64 sequences seqs + off[g] of len[g] >= 13 letters,
 * at most 2^20 in all; ACGT in either case code 0..3, another letter 4.  The
 * index is every 13-mer of valid bases as (kmer, g, pos), sorted, without the
 * k-mers that occur more than 64 times in their target.
 * ccsx_ref_host: the definition as a sequential loop for one read ccs / n
 * (ASCII; n may be 0): writes *rec and, if words is not NULL, its n words (of
 * the read in orientation rec->o).  Returns 0, or -1 for a NULL set or rec.
 * ccsx_ref_pass: 1 iff the read is mapped (g >= 0), aln >= y and
 * 100 mat >= Y aln. */
ccsx_pairaln ccsx_pairwise_band_path(const uint8_t *q, uint32_t qlen, const uint8_t *t, uint32_t tlen, int32_t d0,
                                     uint32_t *words);
ccsx_ref_set *ccsx_ref_set_make(const char *seqs, const uint32_t *off, const uint32_t *len, uint32_t G);
void ccsx_ref_set_free(ccsx_ref_set *set);
int32_t ccsx_ref_host(const ccsx_ref_set *set, const char *ccs, uint32_t n, ccsx_ref_rec *rec, uint32_t *words);
int32_t ccsx_ref_pass(const ccsx_ref_rec *rec, int32_t y, int32_t Y);

/* Synthetic PacBio-like ZMW: insert of length L drawn from
 * splitmix64(seed ^ hole), `passes` full passes on alternating strands with
 * 6% insertions / 3% deletions / 1% substitutions.  Writes the concatenated
 * subreads into out (capacity >= passes * (2L + 16)) and their lengths into
 * lens[passes]; if insert != NULL the true insert (L bytes) is written too.
 * Returns the total number of bases written. */
uint64_t ccsx_synth_zmw(uint64_t seed, uint64_t hole, uint32_t L, uint32_t passes,
                        char *out, uint32_t *lens, char *insert);

/* Benchmarks: n synthetic ZMWs (ccsx_synth_zmw(seed, holes[i], L[i],
 * passes[i]), then ccsx_prepare_apply) made on nthreads threads; the batch
 * owns the data, ccsx_synth_batch_zmws gives the n push lists
 * (ccsx_zmw_in, include/ccsx_gpu.h; seg_rev = ccsx_prepare's flags) ready for
 * ccsx_gpu_run. */
typedef struct ccsx_synth_batch ccsx_synth_batch;
ccsx_synth_batch *ccsx_synth_batch_make(uint64_t seed, const uint64_t *holes, const uint32_t *L,
                                        const uint32_t *passes, uint32_t n, int nthreads);
const ccsx_zmw_in *ccsx_synth_batch_zmws(const ccsx_synth_batch *b);
/* Give every ZMW of the batch synthetic kinetics planes (ccsx_zmw_in::ipd / pw:
 * a code per base from splitmix64 of seed, the ZMW and the base's index). */
void ccsx_synth_batch_kinetics(ccsx_synth_batch *b, uint64_t seed);
void ccsx_synth_batch_free(ccsx_synth_batch *b);

#ifdef __cplusplus
}
#endif
#endif
