// ccsx_align.h -- what the band aligner's kernel (ccsx_align.hip) and its host
// side (ccsx_align.cpp) share: the slice layout in the aligner's arena and the
// launcher.  SPEC.md §8 defines the alignment; DESIGN.md §16 the layout.
#ifndef CCSX_ALIGN_H
#define CCSX_ALIGN_H
#include <stdint.h>

namespace ccsx_aln {

constexpr int kHalfBand = 256;
constexpr int kBand = 2 * kHalfBand + 1;  // 513 cells per query row
constexpr int kCellsPerLane = 9;          // 57 lanes x 9 cells = 513
constexpr int kBandLanes = kBand / kCellsPerLane;
static_assert(kBandLanes * kCellsPerLane == kBand && kBandLanes <= 64, "the band must tile the wave");
// one record row per query row: a 32-bit word per lane (nine 3-bit records:
// the direction in bits 0..1, bit 2 = the bases match), padded to the wave
constexpr uint32_t kRowWords = 64;
constexpr uint32_t kRowBytes = kRowWords * 4;
constexpr uint32_t kTbRows = 32;  // record rows per LDS block of the traceback
// lengths and |d0| below this keep the kernel's 32-bit coordinates (and its
// row << 4 | cell position word) exact; a job beyond runs on the host
constexpr uint32_t kMaxLen = 1u << 27;

// a job of a slice: offsets into the slice's sequence bytes / record words
struct Job {
    uint64_t q_off, t_off;  // bytes from Args::seq
    uint64_t rec_off;       // words from Args::rec (qlen rows of kRowWords)
    uint32_t qlen, tlen;
    int32_t d0;
    uint32_t pad;  // the path variant: the job's first word in Args::words
};

struct Args {
    const Job *jobs;
    const uint8_t *seq;
    uint32_t *rec;
    int32_t *out;  // 10 words per job (ccsx_pairaln)
    uint32_t njobs;
};

// the path variant's (SPEC.md §18): one §11 word per query base, job by job
struct PathArgs : Args {
    uint32_t *words;
};

}  // namespace ccsx_aln

// ccsx_prepare_batch (host/prepare_gpu.cpp) adds its rounds and the second
// pairs it computed in vain to the context's counters (ccsx_gpu_aln_stats)
struct ccsx_aln_ctx;
void ccsx_aln_count(ccsx_aln_ctx *c, uint64_t rounds, uint64_t discarded);

#endif
