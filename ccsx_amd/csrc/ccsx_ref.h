// ccsx_ref.h -- what the reference mapper's kernels (ccsx_ref.hip), its host
// side (ccsx_ref.cpp) and the host definition (host/refmap.cpp) share: the
// set with its 13-mer index, the vote key, and a slice's tables.  SPEC.md §18
// defines the mapping; DESIGN.md §22 the layout.
#ifndef CCSX_REF_H
#define CCSX_REF_H
#include <stdint.h>

#include "ccsx_align.h"

namespace ccsx_ref {

constexpr int kK = 13;                       // §8 step 1
constexpr uint32_t kKmerMask = (1u << (2 * kK)) - 1u;
constexpr int kBinShift = 5;                 // bins of 32 diagonals
constexpr uint32_t kMaxOcc = 64;             // a k-mer with more occurrences in its target is skipped
constexpr uint32_t kMaxSet = 64;             // targets
constexpr uint32_t kMaxLetters = 1u << 20;   // of a whole set
constexpr uint32_t kPosBits = 20;            // an index entry: g << 20 | pos
// the directory: the first table entry of every value of a k-mer's top 16 bits
// (and the table's size at the end): 256 KiB, which stays in L2
constexpr uint32_t kDirShift = 2 * kK - 16;
constexpr uint32_t kDirSize = (1u << 16) + 1u;
// a vote's key: (2 g + o) << 23 | (bin + 2^22); reads below 2^27 bases and
// sets of at most 2^20 letters keep bin within [-2^22, 2^15)
constexpr uint32_t kBinBias = 1u << 22;
constexpr uint32_t kPairShift = 23;
constexpr uint32_t kEmpty = 0xFFFFFFFFu;
constexpr uint32_t kVoteSlots = 4096, kMinVoteSlots = 64;  // of the LDS table
constexpr uint32_t kVoteThreads = 256;

inline uint32_t vote_key(uint32_t pair, int32_t bin) { return pair << kPairShift | (uint32_t)(bin + (int32_t)kBinBias); }

#ifdef CCSX_REF_HOST_API  // (not for the kernels' translation unit)
}  // namespace ccsx_ref
#include <vector>
// the set as ccsx_ref_set_make leaves it (the type the C-ABI names)
struct ccsx_ref_set {
    std::vector<uint8_t> codes;       // every target's codes 0..4, back to back
    std::vector<uint32_t> off, len;   // of target g in codes
    std::vector<uint32_t> kmer, gpos; // the index, sorted by (kmer, g, pos)
    std::vector<uint32_t> dir;        // kDirSize entries
};
namespace ccsx_ref {
#endif

// a read of a slice: its codes at fwd, the reverse complement's at rc (bytes
// from Args::seq); the vote kernel writes rc
struct Read {
    uint64_t fwd, rc;
    uint32_t n, pad;
};

// what the vote kernel leaves per read
struct Vote {
    int32_t g, o, d0, votes, votes2, overflow, pad[2];
};

struct Args {
    // the set, as uploaded
    const uint32_t *kmer, *gpos, *dir;
    const uint32_t *toff, *tlen;  // per target: its codes' bytes from Args::seq, its length
    uint32_t nent, ntarget;
    // the slice
    const Read *reads;
    uint8_t *seq;
    ccsx_aln::Job *jobs;  // laid out by the host: rec_off, pad (= the words' offset); the kernel finishes them
    Vote *votes;
    uint32_t nreads, slots;
};

}  // namespace ccsx_ref

#endif
