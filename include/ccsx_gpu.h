/*
 * ccsx_gpu.h -- batched C-ABI of the MI355X consensus engine.
 *
 * Replaces step 1 of ccsx's 3-stage pipeline (main.c:698-706):
 *
 *     kt_for(p->nthreads, split_subread ? ccs_for2 : ccs_for, in, n_zmws);
 *
 * with one call per chunk of ZMWs.  The caller runs ccs_prepare()
 * (main.c:344-453) and the strand flip (main.c:471-476 / 527-531) on its CPU
 * threads and passes, per ZMW, the strand-normalised segments in push order
 * (template, template-1 .. 0, template+1 .. n-1).  Everything from there
 * (shredding main.c:541-641 or the -P single POA main.c:486-502, i.e. every
 * beg/push/end/tidy_msa_bspoa call, the breakpoint scan and the CCS emission)
 * runs on the GPU.  Scoring is main.c:841-849's (M=2 X=-6 O=-3 E=-2,
 * bandwidth 128); SPEC.md defines the POA.
 *
 * Ownership: input buffers belong to the caller and are only read during the
 * call.  Output CCS strings live in a context-owned arena, valid until the
 * next ccsx_gpu_run / ccsx_gpu_fetch on the same context.
 * Errors: every function returns 0 on success, < 0 on error; the message is
 * ccsx_gpu_error(ctx).  -1 is a context error (allocation, launch): the
 * context's results are void.  ccsx_gpu_run / ccsx_gpu_fetch return -2 when
 * individual ZMWs failed on the device (out[i].status != 0, no CCS); every
 * other ZMW of the call is valid, and the host program skips only the failed
 * ones (the reference has no per-ZMW failure to mirror).
 * Threading: one context per device; a context is used by one host thread.
 */
#ifndef CCSX_GPU_H
#define CCSX_GPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ccsx_ctx ccsx_ctx;

enum { CCSX_MODE_SHRED = 0, CCSX_MODE_PRIMITIVE = 1 };

typedef struct {
    const char *seqs;         /* the ZMW's bases (ASCII), segments are slices of it */
    const uint32_t *seg_off;  /* nseg offsets into seqs, in push order */
    const uint32_t *seg_len;  /* nseg lengths */
    uint32_t nseg;
    const uint8_t *seg_rev;   /* nseg strand flags (1: ccs_prepare marked the segment reverse), or NULL = all
                               * forward; read only with ccsx_gpu_set_pileup, ccsx_gpu_set_kinetics or
                               * ccsx_gpu_set_by_strand on */
    const uint8_t *ipd;       /* the 8-bit inter-pulse duration code of every base, parallel to seqs and in the
                               * orientation the segments are pushed in (SPEC.md section 13), or NULL = none;
                               * read only with ccsx_gpu_set_kinetics on */
    const uint8_t *pw;        /* the pulse width codes, likewise (NULL in either: the ZMW has no kinetics) */
} ccsx_zmw_in;

typedef struct {
    const char *ccs;          /* ASCII CCS (not NUL-terminated), ctx-owned */
    uint32_t len;             /* 0 = no CCS (main.c:713 writes nothing) */
    int32_t status;           /* 0 ok; see ccsx_gpu_status_str */
    uint64_t cells;           /* DP cells computed for this ZMW */
} ccsx_zmw_out;

/* Number of HIP devices visible to this process (0 if none). */
int ccsx_gpu_device_count(void);

/* Open a context on HIP device `device`. */
int ccsx_gpu_open(int device, ccsx_ctx **ctx);
void ccsx_gpu_close(ccsx_ctx *ctx);
const char *ccsx_gpu_error(const ccsx_ctx *ctx);
const char *ccsx_gpu_status_str(int32_t status);

/* One chunk (replaces kt_for(ccs_for2/ccs_for)): stage + launch + fetch, in
 * slices that fit the device memory; a ZMW whose graph outgrows the default
 * (tight) workspace capacities is re-run with exact upper-bound capacities.
 * Returns 0, -2 (some ZMWs failed, see out[i].status) or -1. */
int ccsx_gpu_run(ccsx_ctx *ctx, int mode, const ccsx_zmw_in *z, size_t nz, ccsx_zmw_out *out);

/* Pipelined batches (the host program's step 1): ccsx_gpu_submit stages a
 * batch that fits one slot into a free slot of the context's two and launches
 * it without waiting; ccsx_gpu_collect waits for that slot's batch and
 * returns its results (ZMWs that outgrew a tight cap re-run with full caps
 * inside the collect).  Submitting the next batch before collecting the
 * previous keeps the device fed.  *slot: the ticket to collect.  The
 * caller's input arrays must stay valid until the collect; out[i].ccs is
 * valid until that slot's next collect.  submit returns -3 when both slots
 * hold uncollected batches and -4 when the batch does not fit one slot
 * (ccsx_gpu_slot_bytes; or mixes launch classes): run it with ccsx_gpu_run
 * once the submitted batches are collected (ccsx_gpu_run drops uncollected
 * ones).  collect returns 0, -2 (some ZMWs failed) or -1. */
int ccsx_gpu_slot_bytes(ccsx_ctx *ctx, uint64_t *bytes);
/* Reserve the pinned host staging (subreads, CCS; exactly these sizes, the
 * CCS size twice with ccsx_gpu_set_quality on) of
 * the slot the next submit takes, e.g. on a worker thread while the first
 * batch is still being read, instead of in that batch's staging (huge-page
 * mapping, touch, registration: ~0.1 s per GB).  The other slot's is sized by
 * its first batch, while the first one's kernel runs. */
int ccsx_gpu_reserve_staging(ccsx_ctx *ctx, uint64_t seq_bytes, uint64_t out_bytes);
int ccsx_gpu_submit(ccsx_ctx *ctx, int mode, const ccsx_zmw_in *z, size_t nz, int *slot);
int ccsx_gpu_collect(ccsx_ctx *ctx, int slot, ccsx_zmw_out *out);

/* Contexts sharing one device concurrently (the CLI keeps two chunks in flight
 * per GPU): cap this context's slices at total device memory / share
 * (default 1 = whatever is free). */
int ccsx_gpu_set_mem_share(ccsx_ctx *ctx, uint32_t share);
/* The fraction of the device memory all contexts sharing it may use together
 * (default 0.5; 0.05 < frac <= 0.95): each context's slices are sized from
 * total memory x frac / share, split over its two slots. */
int ccsx_gpu_set_mem_frac(ccsx_ctx *ctx, float frac);
/* on != 0: the first ccsx_gpu_run reserves the whole slice budget for the
 * workspace at once instead of growing it with the chunk size (re-allocating
 * a workspace a launch has touched costs ~30 ms per GB; a fresh one does
 * not).  For long runs such as the CLI's growing chunks. */
int ccsx_gpu_set_prealloc(ccsx_ctx *ctx, int on);

/* -v >= 3 (main.c:619-620): on != 0 makes the following ccsx_gpu_run calls
 * (shredded mode) record, per ZMW and shredding round, the breakpoint i and
 * the MSA's column count (msaidxs->size) that ccs_for2 prints.
 * ccsx_gpu_bp_log: the log of ZMW `zmw` (index into the last ccsx_gpu_run's
 * batch) as nrounds (i, ncols) pairs, ctx-owned until the next run. */
int ccsx_gpu_set_bp_log(ccsx_ctx *ctx, int on);
int ccsx_gpu_bp_log(const ccsx_ctx *ctx, size_t zmw, const uint32_t **pairs, uint32_t *nrounds);
/* Per-base consensus qualities (SPEC.md section 9), off by default.  on != 0:
 * the following ccsx_gpu_stage* / ccsx_gpu_run / ccsx_gpu_submit calls give
 * every ZMW a second output plane, device and pinned host, of one quality byte
 * (0 .. 93, not ASCII) per CCS byte, written by the kernel's emission and
 * copied back with the CCS.  With quality on, ccsx_gpu_zmw_bytes, the batch
 * size ccsx_gpu_submit checks against ccsx_gpu_slot_bytes,
 * ccsx_gpu_staged_bytes and the output size ccsx_gpu_reserve_staging pins
 * include that plane (the ZMW's output slab once more); with quality off they,
 * the kernel's work and the bytes copied are what they are without this call.
 * A batch keeps the setting it was staged or submitted with (the full-capacity
 * re-run inside ccsx_gpu_collect included).  The bspoa-compatible single-POA
 * mode (ccsx_bspoa.h) has no qualities.
 * ccsx_gpu_quality: the qualities of ZMW `zmw` of a batch, *len bytes (= that
 * ZMW's out[i].len; 0 for a ZMW without CCS): slot -1 = the last ccsx_gpu_run
 * or ccsx_gpu_fetch on this context, 0 / 1 = that slot's last collected
 * ccsx_gpu_submit batch.  ctx-owned, valid as long as that batch's out[i].ccs.
 * Returns -1 (ccsx_gpu_error says why) if the batch ran with quality off, is
 * not collected yet, or has no ZMW `zmw`.  The read-level values derived from
 * them are ccsx_qual_rq (ccsx_host.h) and np = the ZMW's nseg. */
int ccsx_gpu_set_quality(ccsx_ctx *ctx, int on);
int ccsx_gpu_quality(ccsx_ctx *ctx, int slot, size_t zmw, const uint8_t **qual, uint32_t *len);
/* Per-pass alignment statistics (SPEC.md section 10), off by default: how each
 * pushed segment lies in the MSA its CCS was called from.  on != 0: the
 * following ccsx_gpu_stage* / ccsx_gpu_run / ccsx_gpu_submit calls give every
 * ZMW one record per segment, in the order of ccsx_zmw_in::seg_off: 24 bytes
 * per segment on the device and in the pinned host output, accumulated by the
 * kernel's emission over the shredding rounds and copied back with the CCS.
 * With pass statistics on, ccsx_gpu_zmw_bytes, the batch size ccsx_gpu_submit
 * checks against ccsx_gpu_slot_bytes and ccsx_gpu_staged_bytes include exactly
 * 24 x nseg per ZMW (a caller sizing ccsx_gpu_reserve_staging adds the same to
 * its out_bytes); with them off those values, the kernel's work and the bytes
 * copied are what they are without this call.  Independent of
 * ccsx_gpu_set_quality.  A batch keeps the setting it was staged or submitted
 * with (the full-capacity re-run inside ccsx_gpu_collect included).  The
 * bspoa-compatible single-POA mode (ccsx_bspoa.h) has no pass statistics.
 * ccsx_gpu_pass_stats: the *nseg records of ZMW `zmw` of a batch: slot -1 =
 * the last ccsx_gpu_run or ccsx_gpu_fetch on this context, 0 / 1 = that slot's
 * last collected ccsx_gpu_submit batch.  ctx-owned, valid as long as that
 * batch's out[i].ccs.  Returns -1 (ccsx_gpu_error says why) if the batch ran
 * with pass statistics off, is not collected yet, has no ZMW `zmw`, or that
 * ZMW failed (status != 0).  cbeg / cend are offsets into the ZMW's CCS;
 * ccsx_pass_identity (ccsx_host.h) derives the identity of a record. */
typedef struct {
    uint32_t match, mismatch, ins, del, cbeg, cend;
} ccsx_pass_stat;
int ccsx_gpu_set_pass_stats(ccsx_ctx *ctx, int on);
int ccsx_gpu_pass_stats(ccsx_ctx *ctx, int slot, size_t zmw, const ccsx_pass_stat **st, uint32_t *nseg);
/* Subread-to-CCS coordinate map (SPEC.md section 11), off by default: where
 * every base of every pushed segment lies in the CCS, as the MSA the CCS was
 * called from places it.  on != 0: the following ccsx_gpu_stage* /
 * ccsx_gpu_run / ccsx_gpu_submit calls give every ZMW one 32-bit word per
 * pushed base: bits 0..29 the offset of the CCS base the subread base is
 * aligned to (or, with CCSX_MAP_INS, of the CCS base it is inserted before;
 * that may be the CCS length), bit 30 (CCSX_MAP_MISMATCH) aligned to a
 * different base, bit 31 (CCSX_MAP_INS) inserted; never both.  4 bytes per
 * base on the device and in the pinned host output, written once per launch by
 * the kernel's emission and copied back with the CCS.  With the map on,
 * ccsx_gpu_zmw_bytes, the batch size ccsx_gpu_submit checks against
 * ccsx_gpu_slot_bytes and ccsx_gpu_staged_bytes include exactly 4 x the sum of
 * seg_len per ZMW -- about four times the subread bytes, so a slice holds
 * fewer ZMWs -- (a caller sizing ccsx_gpu_reserve_staging adds the same to its
 * out_bytes); with it off those values, the kernels launched and the bytes
 * copied are what they are without this call.  Independent of
 * ccsx_gpu_set_quality and ccsx_gpu_set_pass_stats.  A batch keeps the setting
 * it was staged or submitted with (the full-capacity re-run inside
 * ccsx_gpu_collect included).  The bspoa-compatible single-POA mode
 * (ccsx_bspoa.h) has no map.
 * ccsx_gpu_base_map: the *len = seg_len[seg] words of segment `seg` of ZMW
 * `zmw` of a batch, in base order (of the segment as pushed): slot -1 = the
 * last ccsx_gpu_run or ccsx_gpu_fetch on this context, 0 / 1 = that slot's
 * last collected ccsx_gpu_submit batch.  ctx-owned, valid as long as that
 * batch's out[i].ccs.  Returns -1 (ccsx_gpu_error says why) if the batch ran
 * with the map off, is not collected yet, has no ZMW `zmw`, that ZMW failed
 * (status != 0), or seg >= its nseg.  ccsx_map_cigar (ccsx_host.h) derives an
 * alignment from a segment's map. */
#define CCSX_MAP_OFFSET 0x3FFFFFFFu
#define CCSX_MAP_MISMATCH 0x40000000u
#define CCSX_MAP_INS 0x80000000u
int ccsx_gpu_set_base_map(ccsx_ctx *ctx, int on);
int ccsx_gpu_base_map(ccsx_ctx *ctx, int slot, size_t zmw, uint32_t seg, const uint32_t **map, uint32_t *len);
/* Per-base strand pileup (SPEC.md section 12), off by default: the evidence
 * behind every CCS base, as the MSA the CCS was called from holds it, split by
 * the strand of the pushed segments (ccsx_zmw_in::seg_rev; NULL = all forward).
 * on != 0: the following ccsx_gpu_stage* / ccsx_gpu_run / ccsx_gpu_submit calls
 * give every ZMW one 12-byte record per byte of its output slab, device and
 * pinned host -- per strand the reads with A, C, G, T in the base's column, the
 * spanning reads with no base there, and the bases of the dropped columns
 * since the CCS base before; every field saturates at 255 -- written once per
 * launch by the kernel's emission and copied back with the CCS, and a strand
 * flag byte per segment beside them.  With the pileup on, ccsx_gpu_zmw_bytes,
 * the batch size ccsx_gpu_submit checks against ccsx_gpu_slot_bytes and
 * ccsx_gpu_staged_bytes include exactly 12 x the ZMW's output slab + nseg per
 * ZMW (a caller sizing ccsx_gpu_reserve_staging adds the same to its
 * out_bytes); with it off those values, the kernels launched and the bytes
 * copied are what they are without this call.  Independent of
 * ccsx_gpu_set_quality, ccsx_gpu_set_pass_stats and ccsx_gpu_set_base_map.  A
 * batch keeps the setting it was staged or submitted with (the full-capacity
 * re-run inside ccsx_gpu_collect included).  The bspoa-compatible single-POA
 * mode (ccsx_bspoa.h) has no pileup.
 * ccsx_gpu_pileup: the *len (= that ZMW's out[i].len) records of ZMW `zmw` of
 * a batch, record p for CCS base p: slot -1 = the last ccsx_gpu_run or
 * ccsx_gpu_fetch on this context, 0 / 1 = that slot's last collected
 * ccsx_gpu_submit batch.  ctx-owned, valid as long as that batch's out[i].ccs.
 * Returns -1 (ccsx_gpu_error says why) if the batch ran with the pileup off, is
 * not collected yet, has no ZMW `zmw`, or that ZMW failed (status != 0).
 * ccsx_pileup_call (ccsx_host.h) derives a strand's call from a record. */
typedef struct {
    uint8_t fwd[6], rev[6];   /* per strand: A, C, G, T, gap, ins */
} ccsx_pileup;
int ccsx_gpu_set_pileup(ccsx_ctx *ctx, int on);
int ccsx_gpu_pileup(ccsx_ctx *ctx, int slot, size_t zmw, const ccsx_pileup **p, uint32_t *len);
/* Per-base consensus kinetics (SPEC.md section 13), off by default: per CCS
 * base and strand (ccsx_zmw_in::seg_rev; NULL = all forward) the mean
 * inter-pulse duration and pulse width of the pushed bases that carry the
 * consensus base in its column, from the per-base codes ccsx_zmw_in::ipd / pw.
 * on != 0: the following ccsx_gpu_stage* / ccsx_gpu_run / ccsx_gpu_submit calls
 * give every ZMW one 8-byte record per byte of its output slab, device and
 * pinned host -- per strand the 8-bit codes of the two means (ccsx_kin_code,
 * ccsx_host.h) and the number of those bases saturating at 255 -- written once
 * per launch by the kernel's emission and copied back with the CCS; the two
 * code planes of the pushed bases (segment by segment in push order) and a
 * strand byte per segment are staged beside the subreads.  With kinetics on,
 * ccsx_gpu_zmw_bytes, the batch size ccsx_gpu_submit checks against
 * ccsx_gpu_slot_bytes and ccsx_gpu_staged_bytes include exactly 8 x the ZMW's
 * output slab + 2 x the sum of seg_len + nseg per ZMW (a caller sizing
 * ccsx_gpu_reserve_staging adds 8 x the output bytes to its out_bytes); with it
 * off those values, the kernels launched and the bytes copied are what they are
 * without this call, and ipd / pw are not read.  Independent of the other four
 * outputs.  A batch keeps the setting it was staged or submitted with (the
 * full-capacity re-run inside ccsx_gpu_collect included).  A ZMW with ipd or pw
 * NULL gets all-zero records.  The bspoa-compatible single-POA mode
 * (ccsx_bspoa.h) has no kinetics.
 * ccsx_gpu_kinetics: the *len (= that ZMW's out[i].len) records of ZMW `zmw` of
 * a batch, record p for CCS base p: slot -1 = the last ccsx_gpu_run or
 * ccsx_gpu_fetch on this context, 0 / 1 = that slot's last collected
 * ccsx_gpu_submit batch.  ctx-owned, valid as long as that batch's out[i].ccs.
 * Returns -1 (ccsx_gpu_error says why) if the batch ran with kinetics off, is
 * not collected yet, has no ZMW `zmw`, or that ZMW failed (status != 0).
 * ccsx_kinetics_tags (ccsx_host.h) formats a ZMW's records as SAM tags. */
typedef struct {
    uint8_t fwd[3], rev[3];   /* per strand: code of the mean ipd, code of the mean pw, min(reads, 255) */
    uint8_t zero[2];
} ccsx_kinetics;
int ccsx_gpu_set_kinetics(ccsx_ctx *ctx, int on);
int ccsx_gpu_kinetics(ccsx_ctx *ctx, int slot, size_t zmw, const ccsx_kinetics **rec, uint32_t *len);
/* Per-strand consensus (SPEC.md section 14), off by default: the sequence each
 * strand's reads support (ccsx_zmw_in::seg_rev; NULL = all forward), read off
 * the MSA the CCS was called from -- not a second POA over one strand's reads.
 * In every emitted column the strand's reads span, section 6's rule on that
 * strand's counts (the rule ccsx_pileup_call applies to a pileup record) calls
 * a base or a gap; the strand's consensus is the called bases in emission
 * order, columns the joint consensus dropped included, each with section 9's
 * quality from the strand's counts.  Both strands are in the CCS's orientation:
 * nothing is reverse-complemented.
 * on != 0: the following ccsx_gpu_stage* / ccsx_gpu_run / ccsx_gpu_submit calls
 * give every ZMW four bytes per byte of its output slab (bases and qualities of
 * two strands) and two length words, device and pinned host, written once per
 * launch by the kernel's emission and copied back with the CCS, and a strand
 * flag byte per segment beside them.  A strand consensus longer than the tight
 * output slab fails the ZMW like a CCS that is (the full-capacity re-run then
 * holds it: the full slab is at least the pushed bases).  With the output on,
 * ccsx_gpu_zmw_bytes, the batch size ccsx_gpu_submit checks against
 * ccsx_gpu_slot_bytes and ccsx_gpu_staged_bytes include exactly 4 x the ZMW's
 * output slab + nseg + 8 per ZMW (a caller sizing ccsx_gpu_reserve_staging adds
 * the same to its out_bytes); with it off those values, the kernels launched
 * and the bytes copied are what they are without this call.  Independent of the
 * other five outputs.  A batch keeps the setting it was staged or submitted
 * with (the full-capacity re-run inside ccsx_gpu_collect included).  The
 * bspoa-compatible single-POA mode (ccsx_bspoa.h) has no strand consensus.
 * ccsx_gpu_by_strand: the consensus of strand `strand` (0 forward, 1 reverse)
 * of ZMW `zmw` of a batch: *len ASCII bases at *seq (not NUL-terminated) and
 * *len quality bytes (0 .. 93, not ASCII) at *qual; *len = 0 for a strand
 * without a pushed segment.  slot -1 = the last ccsx_gpu_run or ccsx_gpu_fetch
 * on this context, 0 / 1 = that slot's last collected ccsx_gpu_submit batch.
 * ctx-owned, valid as long as that batch's out[i].ccs.  Returns -1
 * (ccsx_gpu_error says why) if the batch ran with the output off, is not
 * collected yet, has no ZMW `zmw`, that ZMW failed (status != 0), or strand is
 * neither 0 nor 1. */
int ccsx_gpu_set_by_strand(ccsx_ctx *ctx, int on);
int ccsx_gpu_by_strand(ccsx_ctx *ctx, int slot, size_t zmw, int strand, const char **seq, const uint8_t **qual,
                       uint32_t *len);
/* The same in three steps (one slice, tight capacities, no re-run), so inputs
 * can stay resident in HBM across launches (used by bench.py).
 * ccsx_gpu_launch returns the kernel time measured with HIP events on the
 * context's stream. */
int ccsx_gpu_stage(ccsx_ctx *ctx, const ccsx_zmw_in *z, size_t nz);
/* ccsx_gpu_stage with the tight capacities ccsx_gpu_run uses for `mode`
 * (shredded: workspaces and the LDS read buffer sized for the pushed windows,
 * not whole segments), so a staged slice runs the same kernel instance a
 * ccsx_gpu_run slice would. */
int ccsx_gpu_stage_for(ccsx_ctx *ctx, int mode, const ccsx_zmw_in *z, size_t nz);
int ccsx_gpu_launch(ccsx_ctx *ctx, int mode, float *kernel_ms);
int ccsx_gpu_fetch(ccsx_ctx *ctx, ccsx_zmw_out *out);

/* Device bytes the staged batch occupies (workspace + arenas; the quality
 * plane, the pass records, the base map, the strand pileup with its strand
 * flags, the kinetics records with their input planes and strand bytes and the
 * by-strand plane with its lengths and strand flags when the batch has them). */
uint64_t ccsx_gpu_staged_bytes(const ccsx_ctx *ctx);

/* Diagnostics: per-phase shader-clock counters (s_memtime) summed over the
 * ZMWs of the last launch: total, read staging, DP, traceback, merge,
 * columns, breakpoint+emission, DP rows.  Off by default.  Only the
 * diagnostic library (libccsx_amd_diag.so) carries the counters: with the
 * product library, turning them on returns -1 (ccsx_gpu_error says why). */
int ccsx_gpu_set_profiling(ccsx_ctx *ctx, int on);
/* Test hook: tight row capacity override (0 = default 3 x longest segment +
 * 4096, the segment capped at the 4,096-base window read buffer in shredded
 * mode). */
int ccsx_gpu_set_tight_rows(ccsx_ctx *ctx, uint32_t rows);
/* Test hook: tight output slab override in bytes (0 = default 2 x longest
 * segment + 1,024; a consensus beyond it re-runs the ZMW with full caps). */
int ccsx_gpu_set_tight_out(ccsx_ctx *ctx, uint32_t bytes);
/* Test hook: tight far slot record rows (0 = default rcap / 16 + 64; a DP
 * meeting more far rows -- more than four predecessors or one beyond the
 * ring -- re-runs the ZMW with full caps, a record per row). */
int ccsx_gpu_set_tight_far(ccsx_ctx *ctx, uint32_t rows);
/* Test hook: half size of the piecewise subread staging (0 = 64 MiB) that a
 * preallocating context sharing its device (ccsx_gpu_set_prealloc,
 * ccsx_gpu_set_mem_share > 1: the CLI's) uses for slices larger than two
 * halves: 128 MiB pinned per slot instead of the whole slice. */
int ccsx_gpu_set_stage_piece(ccsx_ctx *ctx, uint64_t bytes);
/* Kernel configuration of the next slices: -1 (default) = by slice size (the
 * latency configuration 0 -- three waves, 8-row DP blocks, 32-row LDS ring --
 * when it keeps the whole slice resident; for slices of at least 3x what the
 * occupancy one keeps resident a one-wave-per-ZMW configuration with an int16
 * ring: 5 (solo16w, 24 per CU) when the slice's ZMWs average fewer than 64
 * segments, else 4 (solo16, 20 per CU), or 3 (solo, int32 ring) where a
 * pushed read exceeds 16,256 bases or the slice runs the HBM-read instance;
 * else the occupancy configuration 1 -- 4-row blocks, 24-row ring); 0 .. 5
 * force one (2: the throughput configuration, two-wave workgroups, up to 8
 * per CU, only by this call; a forced 4 / 5 the int16 ring cannot take runs 3).
 * ccsx_gpu_kernel_cfg: the configuration of the last staged slice. */
int ccsx_gpu_set_kernel_cfg(ccsx_ctx *ctx, int cfg);
int ccsx_gpu_kernel_cfg(const ccsx_ctx *ctx);
/* ZMWs ccsx_gpu_run has re-run with full caps on this context so far. */
int64_t ccsx_gpu_rerun_count(const ccsx_ctx *ctx);
/* Slices this context has launched on the HBM-read kernel instance so far (the
 * read buffer and the shredding cursors in the workspace, not in LDS: a slice
 * with more than 4,096 segments in a ZMW, or with a segment above 100,000
 * bases unless it is a tight-cap shredded slice).  Read-only; a full-caps
 * re-run is a launch of its own, on either slot. */
int64_t ccsx_gpu_hbm_launches(const ccsx_ctx *ctx);
/* Counters of this context's ccsx_gpu_run calls so far, the first n of:
 * [0] ZMWs re-run with full caps, [1] slices launched, [2] ZMW lists dealt
 * into interleaved parts (a list of one launch class that needs k > 1 slots),
 * [3] the parts of those lists, [4] slices that waited for device memory a
 * neighbour still held, [5] slices cut below the plan to the free memory. */
int ccsx_gpu_run_stats(const ccsx_ctx *ctx, uint64_t *stats, uint32_t n);
/* How long a slice waits for device memory that another context or a just
 * exited process still holds before the call fails (default 60,000 ms).
 * ccsx_gpu_run first cuts its slices to the free memory, then waits only if
 * not even one ZMW fits; a ccsx_gpu_submit batch waits for its whole size. */
int ccsx_gpu_set_mem_wait(ccsx_ctx *ctx, uint32_t ms);
/* Device bytes ZMW *z occupies in a ccsx_gpu_run slice of `mode` (tight
 * capacities: workspace, subreads, output slab -- twice with quality on --,
 * tables, 24 bytes per segment with pass statistics on, 4 bytes per pushed
 * base with the base map on, 12 bytes per output slab byte and one per segment
 * with the strand pileup on, 8 bytes per output slab byte, 2 per pushed base
 * and one per segment with kinetics on, 4 bytes per output slab byte, one per
 * segment and 8 with the by-strand output on). */
uint64_t ccsx_gpu_zmw_bytes(const ccsx_ctx *ctx, int mode, const ccsx_zmw_in *z);
/* Test hook: bytes per slot for ccsx_gpu_run's slices (0 = by device memory:
 * half of this context's share, ccsx_gpu_set_mem_share), so a small batch is
 * cut into several slices. */
int ccsx_gpu_set_slot_budget(ccsx_ctx *ctx, uint64_t bytes);
/* Measurement hooks (the host program maps CCSX_WG_PER_CU / CCSX_SHRED_READ_CAP
 * onto them): pad the LDS request so at most wg_per_cu workgroups share a CU
 * (0 = off); the LDS read buffer of tight-cap shredded slices in bases
 * (1,024-65,536, default 4,096; a longer pushed window re-runs the ZMW with
 * full caps). */
int ccsx_gpu_set_wg_cap(ccsx_ctx *ctx, uint32_t wg_per_cu);
int ccsx_gpu_set_shred_read_cap(ccsx_ctx *ctx, uint32_t bases);
/* Test hook: the next ccsx_gpu_run reports ZMW `zmw` (index into its batch)
 * as failed (status 8) after computing it, as a device failure would; the
 * run returns -2 and the other ZMWs are valid.  -1 = off. */
int ccsx_gpu_set_fault(ccsx_ctx *ctx, int64_t zmw);
int ccsx_gpu_profile(ccsx_ctx *ctx, uint64_t *sums, uint32_t nslots);
/* Diagnostics: the same counters per ZMW (staging order), nslots per ZMW;
 * out holds nzmw * nslots values. */
int ccsx_gpu_profile_zmw(ccsx_ctx *ctx, uint64_t *out, uint32_t nzmw, uint32_t nslots);

/* The band aligner (SPEC.md §8 steps 2-3 on the device, ccsx_align.hip): the
 * banded local alignment ccs_prepare's strand_match needs for abnormal
 * subreads, for many pairs per launch.  Every result equals
 * ccsx_pairwise_band (include/ccsx_host.h) field for field.
 *
 * ccsx_pairaln: an alignment of q[qb, qe) to t[tb, te): matches, mismatches,
 * query bases not in the target (ins), target bases not in the query (del),
 * aligned columns (their sum) and score (+1 / -2 / -2); all zero = none.
 *
 * An aligner context is separate from the consensus contexts: its own stream
 * and its own device arena of at most max_bytes, allocated at the first job
 * and grown as slices need; it takes nothing out of a ccsx_ctx's share (the
 * host program sizes those from CCSX_MEM_FRAC = 0.85 of the device and leaves
 * the rest free).  max_bytes 0 = 4 GiB: about 1,000 pairs of 15 kb per slice
 * (a query base costs 256 bytes of traceback records), and a small part of
 * the 15 % the consensus contexts leave free on a 288 GB device.  The calls on
 * one context are serialised, so several host threads may share it.
 * ccsx_gpu_band_align: n jobs (2-bit codes, values >= 4 never match; the band
 * is the diagonals [d0 - 256, d0 + 256]), cut into slices that fit the arena;
 * a job whose records alone exceed the arena, or whose lengths or |d0| reach
 * 2^30, runs ccsx_pairwise_band on the host with the same result.  kernel_ms
 * (may be NULL) receives the kernels' time by HIP events.  Returns 0 or -1.
 * ccsx_gpu_aln_stats: counters so far, the first min(n, 5) of: [0] jobs,
 * [1] slices launched, [2] jobs run on the host, [3] rounds and [4] second
 * pairs computed but not consulted (both counted by ccsx_prepare_batch). */
typedef struct {
    int32_t qb, qe, tb, te, mat, mis, ins, del, aln, score;
} ccsx_pairaln;
typedef struct ccsx_aln_ctx ccsx_aln_ctx;
typedef struct {
    const uint8_t *q, *t;
    uint32_t qlen, tlen;
    int32_t d0;
} ccsx_band_job;
int ccsx_gpu_aln_open(int device, uint64_t max_bytes, ccsx_aln_ctx **ctx);
void ccsx_gpu_aln_close(ccsx_aln_ctx *ctx);
const char *ccsx_gpu_aln_error(const ccsx_aln_ctx *ctx);
int ccsx_gpu_band_align(ccsx_aln_ctx *ctx, const ccsx_band_job *jobs, size_t n, ccsx_pairaln *out, float *kernel_ms);
int ccsx_gpu_aln_stats(const ccsx_aln_ctx *ctx, uint64_t *stats, uint32_t n);

/* The polisher (SPEC.md §15 on the device, ccsx_polish.hip): every pushed
 * segment of a ZMW is realigned to its finished draft CCS in a 64-cell band
 * guided by the segment's §11 map, the realigned bases vote per draft
 * position, and the polished read is assembled from the votes.  Every result
 * equals ccsx_polish_host (include/ccsx_host.h) byte for byte.
 *
 * ccsx_polish_in: the draft (ccs, len; ASCII), the ZMW's segments as pushed
 * (seqs + seg_off[k], seg_len[k] bytes, ASCII; after the strand flip) and map
 * = their §11 words, segments back to back in push order: what
 * ccsx_gpu_collect and ccsx_gpu_base_map return for a batch that ran with the
 * base map on.  ccsx_polish_out: the polished read (seq, qual: len bytes each,
 * qual 0..kQMax, not ASCII), how it differs from the draft (nsub bases changed,
 * nins inserted, ndel dropped), the realigned map (same layout as the input
 * map, NULL without one) and status: 0, or CCSX_POLISH_BAD_MAP for a map whose
 * offsets decrease within a segment or pass the draft's length (no polished
 * read and no map then; the call's other ZMWs are unaffected).  The pointers
 * belong to the context and hold until its next ccsx_gpu_polish or its close.
 *
 * A polisher context is separate from the consensus contexts and from the
 * aligner's, as the aligner's is: its own stream and its own device arena of
 * at most max_bytes (0 = 4 GiB), allocated at the first call and grown as
 * slices need; a pushed base costs 30 bytes of it and a draft base 49.  The
 * calls on one context are serialised.  ccsx_gpu_polish: nz ZMWs, cut in order
 * into slices that fit the arena; a ZMW that no arena of max_bytes holds, or
 * with a segment or a draft of 2^27 bases or more, runs ccsx_polish_host with
 * the same result.  kernel_ms (may be NULL) receives the three kernels' time
 * by HIP events.  Returns 0 or -1.
 * ccsx_gpu_polish_stats: counters so far, the first min(n, 5) of: [0] ZMWs,
 * [1] segments, [2] slices launched, [3] ZMWs run on the host, [4] ZMWs with a
 * bad map. */
#ifndef CCSX_POLISH_BAD_MAP
#define CCSX_POLISH_BAD_MAP 1
#endif
typedef struct ccsx_polish_ctx ccsx_polish_ctx;
typedef struct {
    const char *ccs;
    uint32_t len;
    const char *seqs;
    const uint32_t *seg_off, *seg_len;
    uint32_t nseg;
    const uint32_t *map;
} ccsx_polish_in;
typedef struct {
    const char *seq;
    const uint8_t *qual;
    uint32_t len, nsub, nins, ndel;
    const uint32_t *map;
    int32_t status;
} ccsx_polish_out;
int ccsx_gpu_polish_open(int device, uint64_t max_bytes, ccsx_polish_ctx **ctx);
void ccsx_gpu_polish_close(ccsx_polish_ctx *ctx);
const char *ccsx_gpu_polish_error(const ccsx_polish_ctx *ctx);
int ccsx_gpu_polish(ccsx_polish_ctx *ctx, const ccsx_polish_in *z, size_t nz, ccsx_polish_out *out, float *kernel_ms);
int ccsx_gpu_polish_stats(const ccsx_polish_ctx *ctx, uint64_t *stats, uint32_t n);

/* The demultiplexer (SPEC.md §16 on the device, ccsx_barcode.hip): every
 * barcode of a set, as given and reverse-complemented, is aligned to both end
 * windows of every CCS read (pattern global, start in the window free, +1 / -2
 * / -2), and per (read, end) the best pattern, its score and end column and
 * the best pattern of another barcode come back.  Every result equals
 * ccsx_barcode_host (include/ccsx_host.h) field for field; ccsx_barcode_call
 * (there) turns a result into the call and the clip lengths.
 *
 * ccsx_bc_in: one CCS read (ASCII; len may be 0).  ccsx_bc_out: e[0] for the
 * window at the read's start, e[1] for the window at the start of its reverse
 * complement, so both are read from the outside inwards: pattern = 2 b + o
 * (barcode b of the set; o = 1: its reverse complement), score, end = the first
 * window column that reaches the score (the clip length at that end), second =
 * the largest score of a pattern of another barcode and second_pattern = the
 * smallest such pattern (CCSX_BC_NONE and -1 for a set of one barcode).
 *
 * A demultiplexer context is separate from the consensus contexts, the
 * aligner's and the polisher's: its own stream, the current set's pattern table
 * (at most 128 KiB) and its own device arena of at most max_bytes (0 = 64 MiB;
 * never less than 1 KiB, one read's share at the widest window), allocated at
 * the first call and grown as slices need; a read costs 2 Wn + 44 bytes of it.
 * The calls on one context are serialised.
 * ccsx_gpu_bc_set: the set for the calls that follow: B sequences (seqs +
 * off[b], len[b] letters ACGT in either case), 1 <= B <= 2048, 1 <= len <= 64,
 * and the window length 1 <= Wn <= 256.  Returns -1, the earlier set kept, for
 * anything else.  Nothing of an earlier set survives a new one.
 * ccsx_gpu_bc_score: nz reads, cut in order into slices that fit the arena;
 * out receives nz results.  kernel_ms (may be NULL) receives the kernel's time
 * by HIP events.  Returns 0, or -1 (also without a set).
 * ccsx_gpu_bc_stats: counters so far, the first min(n, 3) of: [0] reads,
 * [1] slices launched, [2] sets. */
#ifndef CCSX_BC_NONE
#define CCSX_BC_NONE INT32_MIN
#endif
typedef struct ccsx_bc_ctx ccsx_bc_ctx;
typedef struct {
    const char *ccs;
    uint32_t len;
} ccsx_bc_in;
typedef struct {
    int32_t pattern, score, end, second, second_pattern;
} ccsx_bc_end;
typedef struct {
    ccsx_bc_end e[2];
} ccsx_bc_out;
int ccsx_gpu_bc_open(int device, uint64_t max_bytes, ccsx_bc_ctx **ctx);
void ccsx_gpu_bc_close(ccsx_bc_ctx *ctx);
const char *ccsx_gpu_bc_error(const ccsx_bc_ctx *ctx);
int ccsx_gpu_bc_set(ccsx_bc_ctx *ctx, const char *seqs, const uint32_t *off, const uint32_t *len, uint32_t B, uint32_t Wn);
int ccsx_gpu_bc_score(ccsx_bc_ctx *ctx, const ccsx_bc_in *z, size_t nz, ccsx_bc_out *out, float *kernel_ms);
int ccsx_gpu_bc_stats(const ccsx_bc_ctx *ctx, uint64_t *stats, uint32_t n);

/* The adapter scanner (SPEC.md §17 on the device, ccsx_scan.hip): every adapter
 * of a set, as given and reverse-complemented, is aligned with a free start
 * along whole CCS reads (+1 / -2 / -2), and every place of a read where an
 * adapter reaches the threshold comes back as a hit: adapter, orient (1: the
 * reverse complement), the read's bases [start, end) and the score.  The hits
 * equal ccsx_scan_host's (include/ccsx_host.h) field for field; ccsx_scan_cut
 * (there) cuts a read at its hits.
 *
 * ccsx_scan_in: one CCS read (ASCII; len may be 0, at most 16,777,215).
 * ccsx_scan_hit: read = the read's index in the call.
 *
 * A scanner context is separate from every other context: its own stream, the
 * current set's pattern table and its own device arena of at most max_bytes
 * (0 = 256 MiB), allocated at the first call and grown as slices need.  The
 * device emits candidates (read, pattern, column, score) into a buffer of the
 * slice; the host folds the orientations, applies the hit rule, computes the
 * starts and sorts.  A slice whose candidates outnumber its buffer runs once
 * more with the counted capacity; if that does not fit the arena the slice is
 * halved, and a single read that does not fit is scanned by ccsx_scan_host
 * inside the call.  The calls on one context are serialised.
 * ccsx_gpu_scan_set: the set for the calls that follow: A sequences (seqs +
 * off[a], len[a] letters ACGT in either case), 1 <= A <= 64, 1 <= len <= 64,
 * and the threshold 1 <= T <= 100 (per cent of the adapter's length).  Returns
 * -1, the earlier set kept, for anything else.
 * ccsx_gpu_scan: n reads; *hits receives the call's hits sorted by (read, end,
 * adapter), owned by the context until its next call, *nhits their number,
 * kernel_ms (may be NULL) the kernels' time by HIP events.  Returns 0, or -1
 * (also without a set, or for a read longer than 16,777,215).
 * ccsx_gpu_scan_tracks: the same launch with the bottom rows stored (tests and
 * tools): track receives, read after read, S_p(j) as int8 at p * (len + 1) + j
 * for the 2 A patterns, sum over the reads of 2 A (len + 1) bytes in all
 * (track_bytes must be that).  The reads must fit one slice of the arena.
 * ccsx_gpu_scan_tile: the columns a lane emits (TC) and its warm-up (WU) for a
 * set whose longest adapter rounds up to rows (16, 32, 48 or 64); -1 otherwise.
 * ccsx_gpu_scan_stats: counters so far, the first min(n, 6) of: [0] reads,
 * [1] slices launched, [2] sets, [3] candidates, [4] re-runs, [5] reads scanned
 * on the host. */
typedef struct ccsx_scan_ctx ccsx_scan_ctx;
typedef struct {
    const char *ccs;
    uint32_t len;
} ccsx_scan_in;
typedef struct {
    uint32_t read, adapter, orient, start, end;
    int32_t score;
} ccsx_scan_hit;
int ccsx_gpu_scan_open(int device, uint64_t max_bytes, ccsx_scan_ctx **ctx);
void ccsx_gpu_scan_close(ccsx_scan_ctx *ctx);
const char *ccsx_gpu_scan_error(const ccsx_scan_ctx *ctx);
int ccsx_gpu_scan_set(ccsx_scan_ctx *ctx, const char *seqs, const uint32_t *off, const uint32_t *len, uint32_t A, uint32_t T);
int ccsx_gpu_scan(ccsx_scan_ctx *ctx, const ccsx_scan_in *reads, size_t n, const ccsx_scan_hit **hits, uint64_t *nhits,
                  float *kernel_ms);
int ccsx_gpu_scan_tracks(ccsx_scan_ctx *ctx, const ccsx_scan_in *reads, size_t n, int8_t *track, uint64_t track_bytes);
int ccsx_gpu_scan_tile(uint32_t rows, uint32_t *TC, uint32_t *WU);
int ccsx_gpu_scan_stats(const ccsx_scan_ctx *ctx, uint64_t *stats, uint32_t n);

/* The reference mapper (SPEC.md §18 on the device, ccsx_ref.hip and the path
 * variant of ccsx_align.hip): every CCS read is seeded against every sequence
 * of a reference set in both orientations by the 13-mer diagonal vote (§8
 * step 1), the winning (target, orientation) is aligned in the ±256 band (§8
 * steps 2-3), and the alignment's path comes back as one §11 word per base of
 * the oriented read.  Every record and word equals ccsx_ref_host's
 * (include/ccsx_host.h).
 *
 * ccsx_ref_rec: g = the target's index (-1: unmapped, every other field 0),
 * o = 0 the read as given / 1 its reverse complement, d0 = the band's centre
 * diagonal, votes = the winning pair's vote count, votes2 = the largest count
 * of a pair with another target (0: none), a = the band's ten fields on the
 * oriented read.
 *
 * A mapper context is separate from every other context: its own stream, the
 * set (target codes, the sorted 13-mer table and its directory) on the device,
 * one arena of at most max_bytes (0 = 4 GiB) and pinned staging; calls are
 * serialised.  ccsx_gpu_ref_set takes a set made by ccsx_ref_set_make (the
 * context copies what it needs; NULL is refused and the earlier set stays).
 * ccsx_gpu_ref_map: n reads (ASCII), cut in order into slices that fit the
 * arena; per slice one copy in, the vote kernel, the band kernel, one copy
 * out.  recs receives n records; words (may be NULL) the reads' words back to
 * back, sum of len of them.  A read of 2^27 bases or more, one whose records
 * no arena holds, and one whose votes overflow the vote kernel's table run
 * ccsx_ref_host inside the call.  kernel_ms (may be NULL) receives two values:
 * the vote kernels' and the band kernels' time by HIP events.
 * ccsx_gpu_ref_vote_cap: the slots of the vote kernel's table, a power of two
 * in 64 .. 4096 (the default); -1 for another value.
 * ccsx_gpu_ref_stats: counters so far, the first min(n, 6) of: [0] reads,
 * [1] slices launched, [2] sets, [3] reads mapped (g >= 0), [4] reads whose
 * votes overflowed, [5] reads run on the host (the overflowed included). */
typedef struct {
    int32_t g, o, d0, votes, votes2;
    ccsx_pairaln a;
} ccsx_ref_rec;
typedef struct ccsx_ref_set ccsx_ref_set;
typedef struct ccsx_ref_ctx ccsx_ref_ctx;
int ccsx_gpu_ref_open(int device, uint64_t max_bytes, ccsx_ref_ctx **ctx);
void ccsx_gpu_ref_close(ccsx_ref_ctx *ctx);
const char *ccsx_gpu_ref_error(const ccsx_ref_ctx *ctx);
int ccsx_gpu_ref_set(ccsx_ref_ctx *ctx, const ccsx_ref_set *set);
int ccsx_gpu_ref_map(ccsx_ref_ctx *ctx, const ccsx_scan_in *reads, size_t n, ccsx_ref_rec *recs, uint32_t *words,
                     float *kernel_ms);
int ccsx_gpu_ref_vote_cap(ccsx_ref_ctx *ctx, uint32_t slots);
int ccsx_gpu_ref_stats(const ccsx_ref_ctx *ctx, uint64_t *stats, uint32_t n);

#ifdef __cplusplus
}
#endif
#endif
