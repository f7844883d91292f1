// main.cpp -- the C host program: ccsx's CLI and 3-stage pipeline on top of the
// MI355X engine.
//
// Restates main.c:723-870 (options, I/O, chunked pipeline) and step 0 / step 2
// of worker_pipeline (main.c:649-720).  Step 1 -- kt_for(ccs_for2/ccs_for),
// which deals the chunk's ZMWs over CPU threads with work stealing
// (kthread.c:24-46) -- becomes:
//   * ccs_prepare + strand flip on -j CPU threads (main.c:520-536);
//   * the chunk's ZMWs cut into cost-balanced micro-batches in
//     longest-first order (host/dispatch.cpp), queued behind the previous
//     chunk's;
//   * one worker thread per device context pulls batches from the queue and
//     runs them through the batched C-ABI (include/ccsx_gpu.h); two contexts
//     per GPU by default (CCSX_SLOTS), whose batches overlap on the device;
//   * a writer thread emits each chunk in input order once its last batch is
//     back (main.c:707-717).
// A ZMW the device cannot finish is reported on stderr and skipped; the other
// ZMWs of the run are written (the reference has no per-ZMW failure).
#include <errno.h>
#include <getopt.h>
#include <malloc.h>
#include <sys/mman.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_set>
#include <vector>

#include "ccsx_gpu.h"
#include "ccsx_host.h"
#include "ingest.h"

namespace {

// ZMWs the reader takes into the first chunk before it waits for the device
// contexts to fix the chunk sizes
constexpr size_t kChunkProvisional = 16384;

// Bases of a chunk's ZMWs live in one arena per chunk (an anonymous mapping
// with transparent huge pages), recycled through a pool: per-ZMW strings
// (~130 KB each, ~2 GB per 16,384-ZMW chunk) cost a page fault per 4 KB page
// when written and a page-table teardown when freed -- 0.55 s per chunk at
// the process exit, which the CLI's timed run pays for every chunk still held.
class ArenaPool {
public:
    struct Arena {
        char *p = nullptr;
        size_t cap = 0;
    };
    Arena get(size_t need)
    {
        {
            std::lock_guard<std::mutex> g(m_);
            for (size_t i = 0; i < free_.size(); ++i)
                if (free_[i].cap >= need) {
                    Arena a = free_[i];
                    free_.erase(free_.begin() + (long)i);
                    return a;
                }
        }
        Arena a;
        a.cap = std::max<size_t>((need + need / 8 + (2u << 20) - 1) & ~size_t((2u << 20) - 1), 2u << 20);
        void *p = mmap(nullptr, a.cap, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (p == MAP_FAILED) {
            fprintf(stderr, "[ccsx] cannot map %zu bytes for a chunk's bases\n", a.cap);
            std::_Exit(1);
        }
        if (!getenv("CCSX_NO_THP")) (void)madvise(p, a.cap, MADV_HUGEPAGE);
        a.p = static_cast<char *>(p);
        return a;
    }
    // back to the pool; unmapped at once once the input has ended (drain):
    // tearing memory down costs ~50 ms per GB even with huge pages (13 GB of
    // arenas: 0.64 s), which the worker that returns an arena pays while the
    // device still runs the last batches, instead of the process exit
    void put(Arena a)
    {
        if (!a.p) return;
        {
            std::lock_guard<std::mutex> g(m_);
            if (!draining_) {
                free_.push_back(a);
                return;
            }
        }
        munmap(a.p, a.cap);
    }
    void drain()
    {
        std::vector<Arena> v;
        {
            std::lock_guard<std::mutex> g(m_);
            draining_ = true;
            v.swap(free_);
        }
        for (Arena &a : v) munmap(a.p, a.cap);
    }

private:
    std::mutex m_;
    std::vector<Arena> free_;
    bool draining_ = false;
};

struct Zmw {
    ccsx_ingest::ZmwRef ref;  // the subreads as spans of the input blocks (until assembled)
    std::string movie, hole;
    char *seqs = nullptr;     // the bases (in the chunk's arena)
    std::vector<uint32_t> lens;
    std::vector<uint32_t> seg_off, seg_len;
    std::vector<uint8_t> seg_rev;
    std::string ccs;
    std::string qual;         // -q: the CCS bases' qualities, Q + 33
    double rq = 0;            // -q: predicted accuracy of the read (ccsx_qual_rq)
    std::vector<ccsx_pass_stat> pst;  // -r: one record per segment (SPEC.md section 10)
    std::string paf;          // -a: the PAF lines of its segments (SPEC.md section 11)
    std::string sites;        // -s: the lines of its discordant sites (SPEC.md section 12)
    std::string strands;      // -b: the records of its strand consensuses (SPEC.md section 14)
    std::string polished;     // -p: the record of its polished read (SPEC.md section 15)
    std::string demux;        // -B -d: the record of its trimmed read, if assigned (SPEC.md section 16)
    std::string demux_row;    // -B -D: its line of the demultiplexing report
    std::string scan_rows;    // -I -i: the lines of its adapter hits (SPEC.md section 17)
    std::string pieces;       // -I -S: the records of its pieces
    std::vector<uint8_t> kin;  // -k: the ipd codes of its bases, then the pw codes, parallel to seqs (empty: a subread lacks them)
    std::string kinline;      // -k: its SAM line (SPEC.md section 13)
    bool kin_arrays = false;  // -k: ... carries the four arrays
    int32_t status = 0;
    std::vector<uint32_t> bp;  // -v >= 3: (breakpoint, MSA columns) per shredding round
};

struct Chunk {
    size_t id = 0;
    std::vector<Zmw> zs;
    ArenaPool *pool = nullptr;
    ArenaPool::Arena arena;  // the ZMWs' bases (needed until every batch is staged)
    void release_arena()
    {
        if (pool) pool->put(arena);
        arena = ArenaPool::Arena{};
    }
    ~Chunk() { release_arena(); }
    std::atomic<size_t> pending{0};  // batches not yet back from a device
    double t_read0 = 0, t_read1 = 0;  // CCSX_TIMING: when step 0's reader read it
    bool last_input = false;           // the input ended inside this chunk
    const char *input_hi = nullptr;    // end of the last record read into it (ZmwSource::release)
};

struct Batch {
    std::shared_ptr<Chunk> chunk;
    std::vector<uint32_t> idx;  // ZMWs of the chunk
};

int usage()
{
    fprintf(stdout,
            "Program: ccsx\n"
            "Version: 1.0.0 (MI355X engine)\n"
            "Usage  : ccsx  [options] <INPUT> <OUTPUT>\n"
            "Generate circular consensus sequences (ccs) from subreads.\n"
            "\n"
            "Options:\n"
            "-h             Output this help \n"
            "-v             debug \n"
            "-m     <int>   Minimum total length of subreads in a hole to use for generating CCS. [5000] \n"
            "-M     <int>   Maximum total length of subreads in a hole to use for generating CCS. [500000] \n"
            "-c     <int>   Minimum number of subreads required to generate CCS. [3] \n"
            "-A             For fasta/fastq input,gzip allowed  \n"
            "-P             primitive bsalign,subread shred by default \n"
            "-q             Output fastq: per-base consensus qualities (Q+33), np= and rq= in the header \n"
            "-r     <file>  Pass report (tab-separated): per subread, its match/mismatch/ins/del counts against the CCS, the CCS stretch it covers, identity \n"
            "-a     <file>  Subread-to-CCS alignments (PAF, cg:Z: with =/X/I/D): per subread, where its bases lie in the CCS by the alignment the CCS was called from \n"
            "-s     <file>  Strand-discordant sites (tab-separated): per CCS position whose forward and reverse subreads call different bases (or base against gap), the two calls and the per-strand A/C/G/T/gap/ins counts \n"
            "-b     <file>  Per-strand consensus (fasta, fastq with -q): per CCS read the sequence its forward and its reverse subreads support in the alignment the CCS was called from, as <name>/fwd and <name>/rev in the CCS's orientation \n"
            "-p     <file>  Polished reads (fasta, fastq with -q): per CCS read, every subread realigned to the finished CCS on the GPU and the bases voted again per position, as <name>/polished; the main output and the other files stay the draft's \n"
            "-B     <file>  Barcode FASTA (1..2048 sequences of 1..64 ACGT letters): every CCS read's two ends are scored on the GPU against every barcode in both orientations and the read is assigned to a barcode pair \n"
            "-d     <file>  With -B: the assigned reads, barcodes clipped (fasta, fastq with -q), the header extended by bc=<name0>--<name1> bs=<score0>,<score1> bx=<clip0>,<clip1> \n"
            "-D     <file>  With -B: demultiplexing report (tab-separated), one line per CCS read: per end the barcode, orientation, score, runner-up score and clip; the call and why a read is not assigned \n"
            "-W     <int>   With -B: bases of each read end searched for a barcode, 1..256. [96] \n"
            "-T     <int>   With -B: an end is called if its score is at least this percentage of the barcode's length. [60] \n"
            "-L     <int>   With -B: ... and leads the best other barcode's score by at least this. [3] \n"
            "-I     <file>  Adapter FASTA (1..64 sequences of 1..64 ACGT letters): every CCS read is scanned on the GPU, along its whole length, for every adapter in both orientations \n"
            "-i     <file>  With -I: adapter hit report (tab-separated), one line per hit: the read, its length, the adapter, orientation, start, end, score and the adapter's length \n"
            "-S     <file>  With -I: the reads cut at their hits (fasta, fastq with -q): the pieces as <name>/<b>_<e> la=<adapter><+|-> ra=<adapter><+|-> (. at a read's end) \n"
            "-E     <int>   With -I: a place is a hit if its score is at least this percentage of the adapter's length, 1..100. [75] \n"
            "-e     <int>   With -I: the shortest piece -S writes. [50] \n"
            "-k     <file>  Consensus kinetics (unaligned SAM; BAM input only): per CCS read its bases, np/fn/rn and, from the subreads' ip/pw tags, the per-strand mean inter-pulse duration and pulse width per base as fi/fp/ri/rp B:C arrays \n"
            "-X\t\t<str>   Exclude ZMWs from output file,a comma-separated list of ID \n"
            "-j     <int>   Number of CPU threads for subread preparation. [1] \n"
            "\n"
            "Environment:\n"
            "CCSX_NGPU      Number of GPU contexts groups [all visible GPUs]; more than the visible\n"
            "               GPUs places group g on GPU g %% visible (logical contexts)\n"
            "CCSX_SLOTS     Device contexts (worker threads) per group [2]\n"
            "CCSX_ASYNC     0: one ccsx_gpu_run per batch instead of pipelined submit / collect [1]\n"
            "CCSX_TIMING    1: per-chunk / per-batch timing on stderr\n"
            "CCSX_CHUNK     Largest chunk in ZMWs [16384 x contexts; 8192 x contexts with CCSX_ASYNC=0]\n"
            "CCSX_CHUNK0    First chunk in ZMWs [CCSX_CHUNK / 2], growing x4 up to CCSX_CHUNK\n"
            "CCSX_MIN_BATCH Fewest ZMWs per micro-batch of a chunk [256] (measurement and test override)\n"
            "CCSX_KCFG      Force a kernel configuration (0 latency, 1 occupancy, 2 throughput, 3 solo)\n"
            "CCSX_DEV_SHARE Processes sharing each GPU [1] (each context's memory share shrinks)\n"
            "CCSX_MEM_FRAC  Fraction of each GPU's memory its contexts size their slices from [0.85]\n"
            "CCSX_GPU_STRAND 1: the band alignments of abnormal subreads (ccs_prepare's strand check) run\n"
            "               batched per chunk on the first GPU instead of on the -j threads [0]\n"
            "\n"
            "Arguments:\n"
            "input          Input file.\n"
            "output         Output file.\n"
            "\n");
    return 1;
}

// Per ZMW of the chunk, on nthreads threads: the bases assembled from the
// input blocks (the copy step 0 of the reference makes, main.c:674-685), then
// ccs_prepare + strand flip (the CPU half of step 1, main.c:520-536, with its
// -v output)
// With an aligner context (CCSX_GPU_STRAND=1) the middle step runs for the
// whole chunk at once, its band alignments on the device
// (ccsx_prepare_batch); if that fails the chunk is prepared on the host, with
// one warning.
void prepare_chunk(Chunk &ch, int nthreads, int verbose, bool kinetics, ccsx_aln_ctx *aln, bool timing)
{
    std::vector<Zmw> &zs = ch.zs;
    // each ZMW's bases at its offset in the chunk's arena
    std::vector<size_t> at(zs.size() + 1, 0);
    for (size_t i = 0; i < zs.size(); ++i) at[i + 1] = at[i] + zs[i].ref.total();
    ch.arena = ch.pool->get(at.back());
    std::atomic<size_t> next(0);
    // step 0: the bases (and kinetics planes) assembled, the push list sized
    auto assemble = [&](size_t i) {
        Zmw &z = zs[i];
        z.movie = std::move(z.ref.movie);
        z.hole = std::move(z.ref.hole);
        z.seqs = ch.arena.p + at[i];
        z.lens.resize(z.ref.recs.size());
        size_t o = 0;
        for (size_t k = 0; k < z.ref.recs.size(); ++k) {
            const ccsx_ingest::Rec &r = z.ref.recs[k];
            ccsx_ingest::write_bases(r, &z.seqs[o]);
            z.lens[k] = r.len;
            o += r.len;
        }
        if (kinetics) {
            // -k: the two code planes beside the bases, where every subread has them
            bool have = true;
            for (const ccsx_ingest::Rec &r : z.ref.recs) have = have && r.has_kinetics();
            if (have) {
                z.kin.resize(2 * o + 2);
                size_t q = 0;
                for (const ccsx_ingest::Rec &r : z.ref.recs) {
                    ccsx_ingest::write_kinetics(r, z.kin.data() + q, z.kin.data() + o + q);
                    q += r.len;
                }
            }
        }
        ccsx_ingest::ZmwRef().recs.swap(z.ref.recs);
        std::vector<std::shared_ptr<ccsx_ingest::Block>>().swap(z.ref.keep);
        const uint32_t n = (uint32_t)z.lens.size();
        z.seg_off.resize(n);
        z.seg_len.resize(n);
        z.seg_rev.resize(n);
    };
    // step 2: the push list of ns segments applied (strand flip, kinetics
    // reversal, -v output)
    auto finish = [&](size_t i, uint32_t ns, std::string &msg) {
        Zmw &z = zs[i];
        const size_t total = at[i + 1] - at[i];
        z.seg_off.resize(ns);
        z.seg_len.resize(ns);
        z.seg_rev.resize(ns);
        msg.clear();
        if (verbose > 1) msg += "poa begin " + z.hole + "\n";
        for (uint32_t l = 0; l < ns; ++l) {
            if (z.seg_rev[l]) ccsx_revcomp(&z.seqs[z.seg_off[l]], z.seg_len[l]);
            if (z.seg_rev[l] && !z.kin.empty()) {
                // (ccsx_prepare_apply_kin: the values stay with their bases)
                uint8_t *a = z.kin.data() + z.seg_off[l], *b = z.kin.data() + total + z.seg_off[l];
                std::reverse(a, a + z.seg_len[l]);
                std::reverse(b, b + z.seg_len[l]);
            }
            if (verbose) {
                // main.c:477-479 / 533-535
                char h[160];
                snprintf(h, sizeof h, ">%s_%u/%u strand=%d len=%u \n", z.hole.c_str(), l, ns, z.seg_rev[l],
                         z.seg_len[l]);
                msg += h;
                msg.append(z.seqs + z.seg_off[l], z.seg_len[l]);
                msg += '\n';
            }
        }
        if (!msg.empty()) fwrite(msg.data(), 1, msg.size(), stderr);
    };
    auto on_threads = [&](const std::function<void()> &work) {
        std::vector<std::thread> th;
        for (int t = 1; t < nthreads; ++t) th.emplace_back(work);
        work();
        for (auto &t : th) t.join();
    };
    // step 1 on the host: ccs_prepare per ZMW
    auto host_prepare = [&](size_t i) {
        Zmw &z = zs[i];
        return ccsx_prepare(z.seqs, z.lens.data(), (uint32_t)z.lens.size(), z.seg_off.data(), z.seg_len.data(),
                            z.seg_rev.data());
    };
    const auto t0 = std::chrono::steady_clock::now();
    auto since_t0 = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    if (!aln) {
        on_threads([&]() {
            std::string msg;
            for (size_t i; (i = next.fetch_add(1)) < zs.size();) {
                assemble(i);
                finish(i, host_prepare(i), msg);
            }
        });
        if (timing) fprintf(stderr, "[ccsx] chunk %zu prepare: %.1f ms on %d threads\n", ch.id, since_t0(), nthreads);
        return;
    }
    on_threads([&]() {
        for (size_t i; (i = next.fetch_add(1)) < zs.size();) assemble(i);
    });
    const size_t nz = zs.size();
    std::vector<const char *> seqs(nz);
    std::vector<const uint32_t *> lens(nz);
    std::vector<uint32_t> n(nz), nseg(nz, 0);
    std::vector<uint32_t *> so(nz), sl(nz);
    std::vector<uint8_t *> sr(nz);
    for (size_t i = 0; i < nz; ++i) {
        seqs[i] = zs[i].seqs, lens[i] = zs[i].lens.data(), n[i] = (uint32_t)zs[i].lens.size();
        so[i] = zs[i].seg_off.data(), sl[i] = zs[i].seg_len.data(), sr[i] = zs[i].seg_rev.data();
    }
    ccsx_batch_info bi;
    const bool ok = ccsx_prepare_batch(aln, seqs.data(), lens.data(), n.data(), nz, nthreads, so.data(), sl.data(),
                                       sr.data(), nseg.data(), &bi) == 0;
    if (!ok) {
        static std::atomic<bool> warned(false);
        if (!warned.exchange(true))
            fprintf(stderr, "[ccsx] CCSX_GPU_STRAND: the device aligner failed (%s); preparing on the host\n",
                    ccsx_gpu_aln_error(aln));
    } else if (timing) {
        fprintf(stderr,
                "[ccsx] chunk %zu strand check: %llu rounds, %llu jobs, seed %.1f ms, device %.1f ms (kernels %.1f ms), "
                "batched prepare %.1f ms, %.1f ms with the assembly\n",
                ch.id, (unsigned long long)bi.rounds, (unsigned long long)bi.jobs, bi.seed_ms, bi.device_ms, bi.kernel_ms,
                bi.total_ms, since_t0());
    }
    next = 0;
    on_threads([&]() {
        std::string msg;
        for (size_t i; (i = next.fetch_add(1)) < zs.size();) finish(i, ok ? nseg[i] : host_prepare(i), msg);
    });
    if (timing) fprintf(stderr, "[ccsx] chunk %zu prepare: %.1f ms on %d threads\n", ch.id, since_t0(), nthreads);
}

// the batch queue between step 0 and the device workers
class BatchQueue {
public:
    void push(std::vector<Batch> &&bs)
    {
        {
            std::lock_guard<std::mutex> g(m_);
            for (auto &b : bs) q_.push_back(std::move(b));
        }
        cv_.notify_all();
    }
    void close()
    {
        {
            std::lock_guard<std::mutex> g(m_);
            closed_ = true;
        }
        cv_.notify_all();
    }
    bool pop(Batch &b)
    {
        std::unique_lock<std::mutex> g(m_);
        cv_.wait(g, [this] { return closed_ || !q_.empty(); });
        if (q_.empty()) return false;
        b = std::move(q_.front());
        q_.pop_front();
        return true;
    }
    // without waiting: false if no batch is queued right now
    bool try_pop(Batch &b)
    {
        std::lock_guard<std::mutex> g(m_);
        if (q_.empty()) return false;
        b = std::move(q_.front());
        q_.pop_front();
        return true;
    }

private:
    std::mutex m_;
    std::condition_variable cv_;
    std::deque<Batch> q_;
    bool closed_ = false;
};

// chunks of ZMW references from step 0's reader to the preparing thread,
// bounded (reading chunk k + 1 overlaps preparing chunk k); an empty chunk
// ends the input
class ReadQueue {
public:
    explicit ReadQueue(size_t limit) : limit_(limit) {}
    void push(std::shared_ptr<Chunk> c)
    {
        std::unique_lock<std::mutex> g(m_);
        space_.wait(g, [this] { return q_.size() < limit_ || stop_; });
        q_.push_back(std::move(c));
        ready_.notify_all();
    }
    std::shared_ptr<Chunk> pop()
    {
        std::unique_lock<std::mutex> g(m_);
        ready_.wait(g, [this] { return !q_.empty(); });
        auto c = std::move(q_.front());
        q_.pop_front();
        space_.notify_all();
        return c;
    }
    void stop()
    {
        {
            std::lock_guard<std::mutex> g(m_);
            stop_ = true;
        }
        space_.notify_all();
    }

private:
    std::mutex m_;
    std::condition_variable space_, ready_;
    std::deque<std::shared_ptr<Chunk>> q_;
    size_t limit_;
    bool stop_ = false;
};

// chunks in input order, handed from step 0 to the writer; bounded so step 0
// runs at most `limit` chunks ahead of the output
class ChunkRing {
public:
    explicit ChunkRing(size_t limit) : limit_(limit) {}
    void add(const std::shared_ptr<Chunk> &c)
    {
        std::unique_lock<std::mutex> g(m_);
        space_.wait(g, [this] { return q_.size() < limit_ || stop_; });
        q_.push_back(c);
        ready_.notify_all();
    }
    void finish()
    {
        {
            std::lock_guard<std::mutex> g(m_);
            eof_ = true;
        }
        ready_.notify_all();
    }
    void stop()
    {
        {
            std::lock_guard<std::mutex> g(m_);
            stop_ = true;
        }
        space_.notify_all();
        ready_.notify_all();
    }
    void batch_done()
    {
        // the decrement happened outside the lock: take it once so a writer
        // between its predicate check and its wait cannot miss this wake-up
        { std::lock_guard<std::mutex> g(m_); }
        ready_.notify_all();
    }
    // the oldest chunk once every batch of it is back; null at the end
    std::shared_ptr<Chunk> next_done()
    {
        std::unique_lock<std::mutex> g(m_);
        ready_.wait(g, [this] { return stop_ || (!q_.empty() && q_.front()->pending == 0) || (q_.empty() && eof_); });
        if (stop_ || q_.empty()) return nullptr;
        auto c = q_.front();
        return c;
    }
    void pop()
    {
        std::lock_guard<std::mutex> g(m_);
        q_.pop_front();
        space_.notify_all();
    }

private:
    std::mutex m_;
    std::condition_variable space_, ready_;
    std::deque<std::shared_ptr<Chunk>> q_;
    size_t limit_;
    bool eof_ = false, stop_ = false;
};

// -X (main.c:772-782): each option kputs-appends its argument to one buffer,
// then ksplit(',') splits the buffer *as a C string* in place (kstring.c:
// 65-107: a field's end delimiter becomes NUL, empty fields are skipped) and
// a fresh hole set holds the fields.  So only the last -X's set counts, and
// after a first split the buffer's C string ends at the first field: `-X 3,5
// -X 7` excludes hole 3, `-X 3 -X 7` excludes hole 37.
std::unordered_set<std::string> exclude_holes(std::string &buf, const char *arg)
{
    buf.append(arg);
    const size_t l = strnlen(buf.data(), buf.size());
    std::unordered_set<std::string> set;
    std::vector<size_t> starts;
    char last = 0;
    size_t start = 0;
    for (size_t i = 0; i <= l; ++i) {
        const char ch = i < l ? buf[i] : '\0';
        if (ch == ',' || ch == '\0') {
            if (last != 0 && last != ',') {
                if (i < l) buf[i] = '\0';
                starts.push_back(start);
                last = '\0';
                continue;
            }
        } else if (last == ',' || last == 0) {
            start = i;
        }
        last = ch;
    }
    for (size_t st : starts) set.insert(std::string(buf.c_str() + st));
    return set;
}

}  // namespace

// CCSX_CHUNK / CCSX_CHUNK0 (measurement overrides) over the default last
// chunk size cm_def (0: not known yet -- the device count decides it): the
// last and first chunk sizes, computed the same way before and after the
// devices open, the first never above the last.  Unknown sizes
// come back 0.
static void env_chunk_sizes(size_t cm_def, size_t &cm, size_t &c0)
{
    size_t ecm = 0, ec0 = 0;
    if (const char *e = getenv("CCSX_CHUNK")) ecm = std::max<size_t>(1024, strtoull(e, nullptr, 10));
    if (const char *e = getenv("CCSX_CHUNK0")) ec0 = std::min<size_t>(131072, std::max<size_t>(1, strtoull(e, nullptr, 10)));
    cm = ecm ? ecm : cm_def;
    if (ec0) {
        c0 = ecm ? std::min(ec0, ecm) : ec0;
        if (cm) cm = std::max(cm, c0);
    } else {
        c0 = cm ? std::max<size_t>(1024, cm / 2) : 0;
    }
}

int main(int argc, char **argv)
{
    const auto tmain = std::chrono::steady_clock::now();
    // per-ZMW strings (~130 KB of subreads each, a few GB per chunk) from the
    // heap, not one mmap each: freed memory is reused by the next chunk with
    // no munmap / page-fault churn, and nothing is returned to the kernel
    // mid-run (freeing a 16,384-ZMW chunk of mmap'd strings took 0.7 s, and
    // the process exit paid the same for the chunks still held)
    if (!getenv("CCSX_MALLOC_DEFAULT")) {
        mallopt(M_MMAP_THRESHOLD, 32 << 20);
        mallopt(M_TRIM_THRESHOLD, 1 << 30);
    }
    int c, verbose = 0, min_subread_len = 5000, max_subread_len = 500000, min_fulllen_count = 3, nthreads = 1;
    int isbam = 1, split_subread = 1, fastq = 0;
    const char *report_path = nullptr;  // -r
    const char *paf_path = nullptr;     // -a
    const char *site_path = nullptr;    // -s
    const char *kin_path = nullptr;     // -k
    const char *strand_path = nullptr;  // -b
    const char *polish_path = nullptr;  // -p
    const char *bc_path = nullptr;      // -B
    const char *demux_path = nullptr;   // -d
    const char *bcrep_path = nullptr;   // -D
    int bc_window = 96, bc_min_pct = 60, bc_min_lead = 3;  // -W -T -L
    const char *ad_path = nullptr;      // -I
    const char *hit_path = nullptr;     // -i
    const char *piece_path = nullptr;   // -S
    int ad_min_pct = 75, ad_min_piece = 50;  // -E -e
    bool ad_opts = false;               // -E or -e given
    std::unordered_set<std::string> hole_set;
    std::string xbuf;  // -X: kputs-appended, ksplit in place (exclude_holes)
    bool have_holes = false;
    while ((c = getopt(argc, argv, "hm:M:c:j:X:PAvqr:a:s:k:b:p:B:d:D:W:T:L:I:i:S:E:e:")) != -1) {
        switch (c) {
        case 'm': min_subread_len = atoi(optarg); break;
        case 'M': max_subread_len = atoi(optarg); break;
        case 'P': split_subread = 0; break;
        case 'A': isbam = 0; break;
        case 'q': fastq = 1; break;
        case 'r': report_path = optarg; break;
        case 'a': paf_path = optarg; break;
        case 's': site_path = optarg; break;
        case 'k': kin_path = optarg; break;
        case 'b': strand_path = optarg; break;
        case 'p': polish_path = optarg; break;
        case 'B': bc_path = optarg; break;
        case 'd': demux_path = optarg; break;
        case 'D': bcrep_path = optarg; break;
        case 'W': bc_window = atoi(optarg); break;
        case 'T': bc_min_pct = atoi(optarg); break;
        case 'L': bc_min_lead = atoi(optarg); break;
        case 'I': ad_path = optarg; break;
        case 'i': hit_path = optarg; break;
        case 'S': piece_path = optarg; break;
        case 'E': ad_min_pct = atoi(optarg), ad_opts = true; break;
        case 'e': ad_min_piece = atoi(optarg), ad_opts = true; break;
        case 'X':  // main.c:772-782
            have_holes = true;
            hole_set = exclude_holes(xbuf, optarg);
            break;
        case 'c':
            min_fulllen_count = atoi(optarg);
            if (min_fulllen_count < 3) {
                fprintf(stderr, "Error! min fulllen count=[%d] (>=3) !\n", min_fulllen_count);
                return -1;
            }
            break;
        case 'v': verbose++; break;
        case 'j': nthreads = atoi(optarg); break;
        default: return usage();
        }
    }
    if (kin_path && !isbam) {
        fprintf(stderr, "Error! -k needs BAM input (the kinetics are the subreads' ip / pw tags): not with -A\n");
        return 1;
    }
    // -B: the barcode set, read and checked before anything else is opened
    std::vector<std::string> bc_names;
    std::string bc_seqs;
    std::vector<uint32_t> bc_off, bc_len;
    if ((demux_path || bcrep_path) && !bc_path) {
        fprintf(stderr, "Error! -d and -D need a barcode file (-B)\n");
        return 1;
    }
    if (bc_path) {
        if (bc_window < 1 || bc_window > 256) {
            fprintf(stderr, "Error! -W=[%d] (1..256) !\n", bc_window);
            return 1;
        }
        ccsx_barcode_set *bs = ccsx_barcode_read(bc_path);
        const char *const *nm = nullptr, *const *sq = nullptr;
        const uint32_t nb = ccsx_barcode_set_get(bs, &nm, &sq);
        for (uint32_t b = 0; b < nb; ++b) {
            bc_names.push_back(nm[b]);
            bc_off.push_back((uint32_t)bc_seqs.size());
            bc_len.push_back((uint32_t)strlen(sq[b]));
            bc_seqs += sq[b];
        }
        ccsx_barcode_set_free(bs);
        if (!nb || ccsx_barcode_check(bc_seqs.data(), bc_off.data(), bc_len.data(), nb) != 0) {
            fprintf(stderr, "Error! %s is not a barcode file: 1..2048 records of 1..64 ACGT letters\n", bc_path);
            return 1;
        }
    }
    // -I: the adapter set, read and checked before anything else is opened
    std::vector<std::string> ad_names;
    std::string ad_seqs;
    std::vector<uint32_t> ad_off, ad_len;
    if ((hit_path || piece_path || ad_opts) && !ad_path) {
        fprintf(stderr, "Error! -i, -S, -E and -e need an adapter file (-I)\n");
        return 1;
    }
    if (ad_path) {
        if (ad_min_pct < 1 || ad_min_pct > 100) {
            fprintf(stderr, "Error! -E=[%d] (1..100) !\n", ad_min_pct);
            return 1;
        }
        if (ad_min_piece < 0) {
            fprintf(stderr, "Error! -e=[%d] (>=0) !\n", ad_min_piece);
            return 1;
        }
        ccsx_barcode_set *as = ccsx_barcode_read(ad_path);
        const char *const *nm = nullptr, *const *sq = nullptr;
        const uint32_t na = ccsx_barcode_set_get(as, &nm, &sq);
        for (uint32_t a = 0; a < na; ++a) {
            ad_names.push_back(nm[a]);
            ad_off.push_back((uint32_t)ad_seqs.size());
            ad_len.push_back((uint32_t)strlen(sq[a]));
            ad_seqs += sq[a];
        }
        ccsx_barcode_set_free(as);
        if (!na || ccsx_scan_check(ad_seqs.data(), ad_off.data(), ad_len.data(), na, (uint32_t)ad_min_pct) != 0) {
            fprintf(stderr, "Error! %s is not an adapter file: 1..64 records of 1..64 ACGT letters\n", ad_path);
            return 1;
        }
    }
    // main.c:802-826
    const char *in_path = "-";
    FILE *fp_out = nullptr;
    if (argc - optind == 0) {
        fp_out = stdout;
    } else if (argc - optind == 1) {
        in_path = argv[optind];
        fp_out = stdout;
    } else if (argc - optind == 2) {
        in_path = argv[optind];
        fp_out = strcmp(argv[optind + 1], "-") == 0 ? stdout : fopen(argv[optind + 1], "w+");
    } else {
        return usage();
    }
    if (nthreads < 1) nthreads = 1;
    // step 0's input: blocks decompressed ahead on a producer thread (BGZF
    // members inflated on the -j threads), records parsed as spans
    auto rd = ccsx_ingest::ZmwSource::open(in_path, isbam != 0, nthreads);
    if (!rd) {
        fprintf(stderr, "Error: Failed to open infile!\n");
        return 1;
    }
    if (!fp_out) {
        fprintf(stderr, "Cannot open file for write!\n");
        return 1;
    }
    FILE *fp_rep = report_path ? fopen(report_path, "w") : nullptr;
    if (report_path && !fp_rep) {
        fprintf(stderr, "Cannot open file for write!\n");
        return 1;
    }
    FILE *fp_paf = paf_path ? fopen(paf_path, "w") : nullptr;
    if (paf_path && !fp_paf) {
        fprintf(stderr, "Cannot open file for write!\n");
        return 1;
    }
    FILE *fp_site = site_path ? fopen(site_path, "w") : nullptr;
    if (site_path && !fp_site) {
        fprintf(stderr, "Cannot open file for write!\n");
        return 1;
    }
    FILE *fp_kin = kin_path ? fopen(kin_path, "w") : nullptr;
    if (kin_path && !fp_kin) {
        fprintf(stderr, "Cannot open file for write!\n");
        return 1;
    }
    FILE *fp_str = strand_path ? fopen(strand_path, "w") : nullptr;
    if (strand_path && !fp_str) {
        fprintf(stderr, "Cannot open file for write!\n");
        return 1;
    }
    FILE *fp_pol = polish_path ? fopen(polish_path, "w") : nullptr;
    if (polish_path && !fp_pol) {
        fprintf(stderr, "Cannot open file for write!\n");
        return 1;
    }
    FILE *fp_dmx = demux_path ? fopen(demux_path, "w") : nullptr;
    FILE *fp_bcr = bcrep_path ? fopen(bcrep_path, "w") : nullptr;
    if ((demux_path && !fp_dmx) || (bcrep_path && !fp_bcr)) {
        fprintf(stderr, "Cannot open file for write!\n");
        return 1;
    }
    FILE *fp_hit = hit_path ? fopen(hit_path, "w") : nullptr;
    FILE *fp_pcs = piece_path ? fopen(piece_path, "w") : nullptr;
    if ((hit_path && !fp_hit) || (piece_path && !fp_pcs)) {
        fprintf(stderr, "Cannot open file for write!\n");
        return 1;
    }
    if (fp_hit) fprintf(fp_hit, "#name\tlen\tadapter\tstrand\tstart\tend\tscore\talen\n");
    if (fp_bcr)
        fprintf(fp_bcr, "#name\tlen\tbc0\tstrand0\tscore0\tsecond0\tend0\tbc1\tstrand1\tscore1\tsecond1\tend1\tcl\tcr\tcalled0\tcalled1\tassigned\treason\n");
    if (fp_kin) fprintf(fp_kin, "@HD\tVN:1.6\tSO:unknown\n");
    if (fp_rep) fprintf(fp_rep, "#name\tpass\tsbeg\tslen\tmatch\tmismatch\tins\tdel\tcbeg\tcend\tidentity\n");
    // step 1 pipelined per context (ccsx_gpu_submit / ccsx_gpu_collect: the
    // next batch is launched before the previous one is collected);
    // CCSX_ASYNC=0: one ccsx_gpu_run per batch (also for the -v >= 3
    // breakpoint log, which ccsx_gpu_run gathers)
    const bool async = !(getenv("CCSX_ASYNC") && atoi(getenv("CCSX_ASYNC")) == 0) && !(verbose > 2 && split_subread);
    // CCSX_NGPU groups of CCSX_SLOTS contexts; group g on device g % ndev
    // (more groups than devices: logical contexts sharing a device, which is
    // how the multi-GPU split is exercised on a one-GPU box).  Two contexts
    // per GPU: each pulls micro-batches on its own worker thread, so one
    // batch's staging and tail overlap the other's kernels (100k config-E
    // ZMWs: 10.66 s vs 12.12 s with one, profiles/r03); pipelined, each keeps
    // two launches in flight (200k config-E ZMWs: 9.4-9.7 s with two
    // contexts, 10.7 s with one, 9.9-10.0 s for two contexts of ccsx_gpu_run;
    // gpurun_out r04r/r04s)
    int nslot = 2;
    if (const char *e = getenv("CCSX_SLOTS")) nslot = std::max(1, std::min(8, atoi(e)));
    // processes sharing each device (bench.py's multi-rank rehearsal on one
    // GPU): each context's memory share shrinks by that factor
    int dev_share = 1;
    if (const char *e = getenv("CCSX_DEV_SHARE")) dev_share = std::max(1, std::min(64, atoi(e)));
    // measurement overrides of the engine (never set by default)
    const int kcfg = getenv("CCSX_KCFG") ? atoi(getenv("CCSX_KCFG")) : -1;
    const int wg_cap = getenv("CCSX_WG_PER_CU") ? atoi(getenv("CCSX_WG_PER_CU")) : 0;
    const int read_cap = getenv("CCSX_SHRED_READ_CAP") ? atoi(getenv("CCSX_SHRED_READ_CAP")) : 0;
    // the contexts size their slices from 85 % of the device memory (the
    // library's default is half): a context's 8,192-ZMW batch of a config-E
    // chunk then runs as one launch instead of two of 4,096, whose
    // longest-first order balances better (200k config-E ZMWs 11.0 s -> 10.0 s,
    // gpurun_out r04q); CCSX_MEM_FRAC overrides
    const float mem_frac = getenv("CCSX_MEM_FRAC") ? (float)atof(getenv("CCSX_MEM_FRAC")) : 0.85f;
    // micro-batches per context and chunk (CCSX_CTX_BATCHES, default 1: 100k
    // config-E ZMWs from the generator's pipe 15.2 s with 2, 11.8 s with 1,
    // r03o)
    uint32_t batches_per_ctx = 1;
    if (const char *e = getenv("CCSX_CTX_BATCHES")) batches_per_ctx = (uint32_t)std::max(1, std::min(64, atoi(e)));
    // consumed input pages unmapped as chunks are prepared (CCSX_INPUT_RELEASE=0: at the exit)
    const bool input_release = !(getenv("CCSX_INPUT_RELEASE") && atoi(getenv("CCSX_INPUT_RELEASE")) == 0);
    // a context with no more work releases its memory while the others run
    // (CCSX_EARLY_CLOSE=0: the exit releases everything)
    const bool early_close = !(getenv("CCSX_EARLY_CLOSE") && atoi(getenv("CCSX_EARLY_CLOSE")) == 0);
    // the last context too, while the writer emits the last chunks: the exit
    // then has less to release (62,500 config-E ZMWs at -j 8: 317-321 ms from
    // the last batch to the exit against 345-369, r06j; CCSX_LAST_CLOSE=0: off)
    const bool last_close = !(getenv("CCSX_LAST_CLOSE") && atoi(getenv("CCSX_LAST_CLOSE")) == 0);
    // the chunk the input ends in: batches per context (the run ends on its
    // slowest batch; smaller ones let the contexts end together)
    uint32_t last_batches_per_ctx = 1;
    if (const char *e = getenv("CCSX_LAST_BATCHES")) last_batches_per_ctx = (uint32_t)std::max(1, std::min(64, atoi(e)));
    // the fewest ZMWs a micro-batch holds (ccsx_partition's floor; CCSX_MIN_BATCH:
    // a measurement and test override, so that a small input still spreads
    // over several batches per chunk)
    uint32_t min_batch = 256;
    if (const char *e = getenv("CCSX_MIN_BATCH")) min_batch = (uint32_t)std::max(1, atoi(e));
    const bool timing = getenv("CCSX_TIMING") && atoi(getenv("CCSX_TIMING"));
    const bool gpu_strand = getenv("CCSX_GPU_STRAND") && atoi(getenv("CCSX_GPU_STRAND"));
    ccsx_aln_ctx *aln = nullptr;
    // -p: the one polisher context, on the first GPU; its results hold until
    // its next call, so a worker keeps pol_m from its call until it has copied them
    ccsx_polish_ctx *pol = nullptr;
    std::mutex pol_m;
    // -B: the one demultiplexer context, on the first GPU (its calls copy their results out)
    ccsx_bc_ctx *bc = nullptr;
    // -I: the one scanner context, on the first GPU; its hits hold until its
    // next call, so a worker keeps scan_m from its call until it has used them
    ccsx_scan_ctx *scn = nullptr;
    std::mutex scan_m;
    bool aln_tried = false;
    const auto tstart = std::chrono::steady_clock::now();
    auto now_ms = [tstart]() {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tstart).count();
    };
    const int mode = split_subread ? CCSX_MODE_SHRED : CCSX_MODE_PRIMITIVE;
    // the device contexts, opened on their own thread (below) while step 0
    // reads and prepares the first chunk
    int nctx = 0;
    std::vector<ccsx_ctx *> ctx;
    uint64_t slot_bytes = 0;

    ArenaPool arenas;  // (declared before every holder of a chunk)
    BatchQueue queue;
    ChunkRing ring(3);
    std::atomic<bool> fatal(false);
    std::atomic<uint64_t> cells_total(0);  // DP cells the devices computed (CCSX_TIMING report)
    std::atomic<int> workers_busy(0);      // pipelined workers still running
    std::mutex err_m;

    // test hook: the device reports this hole as failed (tests/test_gpu_cli.py)
    const std::string fault_hole = getenv("CCSX_FAULT_HOLE") ? getenv("CCSX_FAULT_HOLE") : "";
    // test hook: batches after the first CCSX_FATAL_AFTER ones fail as a
    // context error does (the fatal path's teardown, tests/test_gpu_cli.py)
    const long fatal_after = getenv("CCSX_FATAL_AFTER") ? atol(getenv("CCSX_FATAL_AFTER")) : -1;
    std::atomic<long> batches_seen(0);

    // step 1, device side: one worker per context
    // a batch in flight on a context: its input arrays live until collected
    struct Flight {
        Batch b;
        std::vector<ccsx_zmw_in> in;
        std::vector<ccsx_zmw_out> out;
        int slot = -1;
        double t0 = 0;
    };
    auto prepare_in = [&](int w, Flight &f) {
        Chunk &ch = *f.b.chunk;
        f.in.resize(f.b.idx.size());
        f.out.assign(f.b.idx.size(), ccsx_zmw_out{});
        for (size_t i = 0; i < f.b.idx.size(); ++i) {
            const Zmw &z = ch.zs[f.b.idx[i]];
            f.in[i] = ccsx_zmw_in{z.seqs, z.seg_off.data(), z.seg_len.data(), (uint32_t)z.seg_len.size(), z.seg_rev.data()};
            if (!z.kin.empty()) f.in[i].ipd = z.kin.data(), f.in[i].pw = z.kin.data() + (z.kin.size() - 2) / 2;
            if (!fault_hole.empty() && z.hole == fault_hole) ccsx_gpu_set_fault(ctx[w], (int64_t)i);
        }
        f.t0 = now_ms();
    };
    // results of a batch (r: the run / collect status) into its chunk
    auto finish = [&](int w, Flight &f, int r) {
        Chunk &ch = *f.b.chunk;
        if (fatal_after >= 0 && batches_seen.fetch_add(1) >= fatal_after) r = -9;
        bool qfail = false;  // -q / -r / -a / -s / -k / -b: the batch's qualities, pass records, maps, pileups, kinetics or strand consensuses are missing (a context error)
        if (r == 0 || r == -2) {
            // -2: some ZMWs failed on the device, the rest are valid
            uint64_t cells = 0;
            for (size_t i = 0; i < f.b.idx.size(); ++i) cells += f.out[i].cells;
            cells_total += cells;
            for (size_t i = 0; i < f.b.idx.size(); ++i) {
                Zmw &z = ch.zs[f.b.idx[i]];
                z.status = f.out[i].status;
                if (!f.out[i].status) z.ccs.assign(f.out[i].ccs, f.out[i].len);
                if (fastq && !f.out[i].status) {
                    // (f.slot: the collected slot, -1 for a batch ccsx_gpu_run ran)
                    const uint8_t *q = nullptr;
                    uint32_t ql = 0;
                    if (ccsx_gpu_quality(ctx[w], f.slot, i, &q, &ql) != 0 || ql != f.out[i].len) {
                        qfail = true;
                        break;
                    }
                    z.rq = ccsx_qual_rq(q, ql);
                    z.qual.resize(ql);
                    for (uint32_t k = 0; k < ql; ++k) z.qual[k] = (char)(q[k] + 33);
                }
                if (fp_rep && !f.out[i].status) {
                    const ccsx_pass_stat *st = nullptr;
                    uint32_t ns = 0;
                    if (ccsx_gpu_pass_stats(ctx[w], f.slot, i, &st, &ns) != 0 || ns != z.seg_len.size()) {
                        qfail = true;
                        break;
                    }
                    z.pst.assign(st, st + ns);
                }
                if (fp_paf && !f.out[i].status) {
                    // one PAF line per segment with an aligned base; query
                    // coordinates on the subread's own strand, CIGAR in CCS order
                    std::string cg;
                    char head[160];
                    for (size_t k = 0; k < z.seg_len.size() && !qfail; ++k) {
                        const uint32_t *mp = nullptr;
                        uint32_t ml = 0;
                        if (ccsx_gpu_base_map(ctx[w], f.slot, i, (uint32_t)k, &mp, &ml) != 0 || ml != z.seg_len[k]) {
                            qfail = true;
                            break;
                        }
                        ccsx_map_aln a;
                        const long n = ccsx_map_cigar(mp, ml, &a, nullptr, 0);
                        if (n < 0) continue;
                        cg.resize((size_t)n + 1);
                        (void)ccsx_map_cigar(mp, ml, &a, &cg[0], cg.size());
                        cg.resize((size_t)n);
                        const bool rev = z.seg_rev[k] != 0;
                        snprintf(head, sizeof head, "/%zu\t%u\t%u\t%u\t%c\t", k, ml, rev ? ml - a.qe : a.qs, rev ? ml - a.qs : a.qe,
                                 rev ? '-' : '+');
                        z.paf += z.movie + "/" + z.hole + head + z.movie + "/" + z.hole + "/ccs";
                        snprintf(head, sizeof head, "\t%u\t%u\t%u\t%u\t%u\t255\tsb:i:%u\tcg:Z:", f.out[i].len, a.ts, a.te, a.n_eq,
                                 a.n_eq + a.n_x + a.n_ins + a.n_del, z.seg_off[k]);
                        z.paf += head;
                        z.paf += cg;
                        z.paf += '\n';
                    }
                    if (qfail) break;
                }
                if (fp_site && !f.out[i].status) {
                    // one line per position whose two strands call differently
                    const ccsx_pileup *pu = nullptr;
                    uint32_t pl = 0;
                    if (ccsx_gpu_pileup(ctx[w], f.slot, i, &pu, &pl) != 0 || pl != f.out[i].len) {
                        qfail = true;
                        break;
                    }
                    char line[160];
                    for (uint32_t p = 0; p < pl; ++p) {
                        const int cf = ccsx_pileup_call(&pu[p], 0), cr = ccsx_pileup_call(&pu[p], 1);
                        if (cf < 0 || cr < 0 || cf == cr) continue;
                        const uint8_t *a = pu[p].fwd, *b = pu[p].rev;
                        snprintf(line, sizeof line, "/ccs\t%u\t%c\t%c\t%c\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\n", p,
                                 f.out[i].ccs[p], "ACGT-"[cf], "ACGT-"[cr], a[0], a[1], a[2], a[3], a[4], a[5], b[0], b[1], b[2],
                                 b[3], b[4], b[5]);
                        z.sites += z.movie + "/" + z.hole + line;
                    }
                }
                if (fp_kin && !f.out[i].status && f.out[i].len) {
                    // the ZMW's SAM line; the four arrays only where it came with kinetics
                    const ccsx_kinetics *kr = nullptr;
                    uint32_t kl = 0;
                    if (ccsx_gpu_kinetics(ctx[w], f.slot, i, &kr, &kl) != 0 || kl != f.out[i].len) {
                        qfail = true;
                        break;
                    }
                    size_t nrev = 0;
                    for (uint8_t v : z.seg_rev) nrev += v != 0;
                    char num[96];
                    std::string &s = z.kinline;
                    s = z.movie + "/" + z.hole + "/ccs\t4\t*\t0\t255\t*\t*\t0\t0\t";
                    s.append(f.out[i].ccs, f.out[i].len);
                    s += '\t';
                    if (fastq) s += z.qual;
                    else s += '*';
                    snprintf(num, sizeof num, "\tnp:i:%zu", z.seg_len.size());
                    s += num;
                    if (fastq) {
                        snprintf(num, sizeof num, "\trq:f:%.6f", z.rq);
                        s += num;
                    }
                    snprintf(num, sizeof num, "\tfn:i:%zu\trn:i:%zu", z.seg_rev.size() - nrev, nrev);
                    s += num;
                    z.kin_arrays = !z.kin.empty();
                    if (z.kin_arrays) {
                        const long n = ccsx_kinetics_tags(kr, kl, nullptr, 0);
                        const size_t at = s.size() + 1;
                        s += '\t';
                        s.resize(at + (size_t)n + 1);
                        (void)ccsx_kinetics_tags(kr, kl, &s[at], (size_t)n + 1);
                        s.resize(at + (size_t)n);
                    }
                    s += '\n';
                    std::vector<uint8_t>().swap(z.kin);
                }
                if (fp_str && !f.out[i].status && f.out[i].len) {
                    // the forward, then the reverse strand's record, laid out as the main output's
                    char head[96];
                    for (int sd = 0; sd < 2 && !qfail; ++sd) {
                        const char *sq = nullptr;
                        const uint8_t *q = nullptr;
                        uint32_t sn = 0;
                        if (ccsx_gpu_by_strand(ctx[w], f.slot, i, sd, &sq, &q, &sn) != 0) {
                            qfail = true;
                            break;
                        }
                        if (!sn) continue;
                        size_t np = 0;
                        for (uint8_t v : z.seg_rev) np += (v != 0) == (sd != 0);
                        std::string &s = z.strands;
                        s += fastq ? '@' : '>';
                        s += z.movie + "/" + z.hole + (sd ? "/ccs/rev" : "/ccs/fwd");
                        if (fastq) {
                            snprintf(head, sizeof head, " np=%zu rq=%.6f", np, ccsx_qual_rq(q, sn));
                            s += head;
                        }
                        s += '\n';
                        s.append(sq, sn);
                        s += '\n';
                        if (fastq) {
                            s += "+\n";
                            for (uint32_t k = 0; k < sn; ++k) s += (char)(q[k] + 33);
                            s += '\n';
                        }
                    }
                    if (qfail) break;
                }
                const uint32_t *lg;
                uint32_t nr = 0;
                if (verbose > 2 && !f.out[i].status && ccsx_gpu_bp_log(ctx[w], i, &lg, &nr) == 0)
                    z.bp.assign(lg, lg + 2 * (size_t)nr);
            }
            if (pol && !qfail) {
                // -p: the batch's ZMWs with a CCS, their drafts and maps as collected
                std::vector<ccsx_polish_in> pin;
                std::vector<size_t> who;
                std::vector<std::vector<uint32_t>> maps;
                for (size_t i = 0; i < f.b.idx.size() && !qfail; ++i) {
                    Zmw &z = ch.zs[f.b.idx[i]];
                    if (f.out[i].status || z.ccs.empty()) continue;
                    std::vector<uint32_t> m;
                    for (size_t k = 0; k < z.seg_len.size(); ++k) {
                        const uint32_t *mp = nullptr;
                        uint32_t ml = 0;
                        if (ccsx_gpu_base_map(ctx[w], f.slot, i, (uint32_t)k, &mp, &ml) != 0 || ml != z.seg_len[k]) {
                            qfail = true;
                            break;
                        }
                        m.insert(m.end(), mp, mp + ml);
                    }
                    pin.push_back(ccsx_polish_in{z.ccs.data(), (uint32_t)z.ccs.size(), z.seqs, z.seg_off.data(), z.seg_len.data(),
                                                 (uint32_t)z.seg_len.size(), nullptr});
                    who.push_back(f.b.idx[i]);
                    maps.push_back(std::move(m));
                }
                for (size_t i = 0; i < pin.size(); ++i) pin[i].map = maps[i].data();
                if (!qfail && !pin.empty()) {
                    std::vector<ccsx_polish_out> po(pin.size());
                    std::lock_guard<std::mutex> g(pol_m);
                    if (ccsx_gpu_polish(pol, pin.data(), pin.size(), po.data(), nullptr) != 0) {
                        std::lock_guard<std::mutex> g2(err_m);
                        fprintf(stderr, "[ccsx] polisher: %s\n", ccsx_gpu_polish_error(pol));
                        qfail = true;
                    }
                    for (size_t i = 0; i < pin.size() && !qfail; ++i) {
                        Zmw &z = ch.zs[who[i]];
                        if (po[i].status || !po[i].len) continue;  // (a collected map is never a bad one)
                        std::string &s = z.polished;
                        s += fastq ? '@' : '>';
                        s += z.movie + "/" + z.hole + "/ccs/polished\n";
                        s.append(po[i].seq, po[i].len);
                        s += '\n';
                        if (fastq) {
                            s += "+\n";
                            for (uint32_t k = 0; k < po[i].len; ++k) s += (char)(po[i].qual[k] + 33);
                            s += '\n';
                        }
                    }
                }
            }
            if (bc && !qfail) {
                // -B: the batch's CCS reads are scored here; then the call, the trimmed record and the report line
                std::vector<ccsx_bc_in> bin;
                std::vector<size_t> who;
                for (size_t i = 0; i < f.b.idx.size(); ++i) {
                    const Zmw &z = ch.zs[f.b.idx[i]];
                    if (f.out[i].status || z.ccs.empty()) continue;
                    bin.push_back(ccsx_bc_in{z.ccs.data(), (uint32_t)z.ccs.size()});
                    who.push_back(f.b.idx[i]);
                }
                std::vector<ccsx_bc_out> bo(bin.size());
                if (!bin.empty() && ccsx_gpu_bc_score(bc, bin.data(), bin.size(), bo.data(), nullptr) != 0) {
                    std::lock_guard<std::mutex> g2(err_m);
                    fprintf(stderr, "[ccsx] demultiplexer: %s\n", ccsx_gpu_bc_error(bc));
                    qfail = true;
                }
                static const char *const why[] = {"ok", "end0", "end1", "ends", "insert"};
                for (size_t i = 0; i < bin.size() && !qfail; ++i) {
                    Zmw &z = ch.zs[who[i]];
                    const uint32_t n = (uint32_t)z.ccs.size();
                    ccsx_bc_call call;
                    ccsx_barcode_call(&bo[i], bc_len.data(), (uint32_t)bc_len.size(), n, bc_min_pct, bc_min_lead, &call);
                    const ccsx_bc_end *e = bo[i].e;
                    char num[160];
                    if (fp_bcr) {
                        std::string &s = z.demux_row;
                        snprintf(num, sizeof num, "/ccs\t%u", n);
                        s = z.movie + "/" + z.hole + num;
                        for (int k = 0; k < 2; ++k) {
                            s += '\t' + bc_names[(size_t)e[k].pattern >> 1];
                            const char o = (e[k].pattern & 1) ? '-' : '+';
                            if (e[k].second_pattern < 0) snprintf(num, sizeof num, "\t%c\t%d\t.\t%d", o, e[k].score, e[k].end);
                            else snprintf(num, sizeof num, "\t%c\t%d\t%d\t%d", o, e[k].score, e[k].second, e[k].end);
                            s += num;
                        }
                        snprintf(num, sizeof num, "\t%u\t%u\t%d\t%d\t%d\t%s\n", call.cl, call.cr, call.called[0], call.called[1],
                                 call.assigned, why[call.reason]);
                        s += num;
                    }
                    if (fp_dmx && call.assigned) {
                        // the read's own header, then the pair, the two scores and the two clips
                        std::string &s = z.demux;
                        s += fastq ? '@' : '>';
                        s += z.movie + "/" + z.hole + "/ccs";
                        if (fastq) {
                            snprintf(num, sizeof num, " np=%zu rq=%.6f", z.seg_len.size(), z.rq);
                            s += num;
                        }
                        s += " bc=" + bc_names[(size_t)e[0].pattern >> 1] + "--" + bc_names[(size_t)e[1].pattern >> 1];
                        snprintf(num, sizeof num, " bs=%d,%d bx=%u,%u\n", e[0].score, e[1].score, call.cl, call.cr);
                        s += num;
                        s.append(z.ccs, call.cl, n - call.cl - call.cr);
                        s += '\n';
                        if (fastq) {
                            s += "+\n";
                            s.append(z.qual, call.cl, n - call.cl - call.cr);
                            s += '\n';
                        }
                    }
                }
            }
            if (scn && !qfail) {
                // -I: the batch's CCS reads are scanned here; then the report lines and the pieces
                std::vector<ccsx_scan_in> sin;
                std::vector<size_t> who;
                for (size_t i = 0; i < f.b.idx.size(); ++i) {
                    const Zmw &z = ch.zs[f.b.idx[i]];
                    if (f.out[i].status || z.ccs.empty()) continue;
                    sin.push_back(ccsx_scan_in{z.ccs.data(), (uint32_t)z.ccs.size()});
                    who.push_back(f.b.idx[i]);
                }
                std::lock_guard<std::mutex> gs(scan_m);
                const ccsx_scan_hit *hits = nullptr;
                uint64_t nhits = 0;
                if (!sin.empty() && ccsx_gpu_scan(scn, sin.data(), sin.size(), &hits, &nhits, nullptr) != 0) {
                    std::lock_guard<std::mutex> g2(err_m);
                    fprintf(stderr, "[ccsx] scanner: %s\n", ccsx_gpu_scan_error(scn));
                    qfail = true;
                }
                std::vector<ccsx_scan_piece> pcs;
                uint64_t h0 = 0;
                for (size_t i = 0; i < sin.size() && !qfail; ++i) {
                    Zmw &z = ch.zs[who[i]];
                    const uint32_t n = (uint32_t)z.ccs.size();
                    uint64_t h1 = h0;
                    while (h1 < nhits && hits[h1].read == i) ++h1;
                    const ccsx_scan_hit *h = hits + h0;
                    const uint64_t nh = h1 - h0;
                    h0 = h1;
                    char num[160];
                    const std::string name = z.movie + "/" + z.hole + "/ccs";
                    if (fp_hit)
                        for (uint64_t k = 0; k < nh; ++k) {
                            snprintf(num, sizeof num, "\t%c\t%u\t%u\t%d\t%u\n", h[k].orient ? '-' : '+', h[k].start, h[k].end,
                                     h[k].score, ad_len[h[k].adapter]);
                            z.scan_rows += name + '\t' + std::to_string(n) + '\t' + ad_names[h[k].adapter] + num;
                        }
                    if (fp_pcs) {
                        const int64_t np = ccsx_scan_cut(h, nh, n, (uint32_t)ad_min_piece, nullptr, 0);
                        pcs.resize((size_t)np);
                        ccsx_scan_cut(h, nh, n, (uint32_t)ad_min_piece, pcs.data(), (uint64_t)np);
                        auto flank = [&](int32_t k) {
                            return k < 0 ? std::string(".") : ad_names[h[k].adapter] + (h[k].orient ? '-' : '+');
                        };
                        for (const ccsx_scan_piece &p : pcs) {
                            std::string &s = z.pieces;
                            snprintf(num, sizeof num, "/%u_%u", p.b, p.e);
                            s += fastq ? '@' : '>';
                            s += name + num + " la=" + flank(p.left) + " ra=" + flank(p.right) + '\n';
                            s.append(z.ccs, p.b, p.e - p.b);
                            s += '\n';
                            if (fastq) {
                                s += "+\n";
                                s.append(z.qual, p.b, p.e - p.b);
                                s += '\n';
                            }
                        }
                    }
                }
            }
        }
        if ((qfail || (r != 0 && r != -2)) && !fatal.exchange(true)) {
            std::lock_guard<std::mutex> g(err_m);
            fprintf(stderr, "[ccsx] device context %d: %s\n", w, r == -9 ? "injected fatal error (test hook)" : ccsx_gpu_error(ctx[w]));
        }
        if (timing)
            fprintf(stderr, "[ccsx] chunk %zu batch of %zu ZMWs on context %d: %.0f-%.0f ms\n", ch.id, f.b.idx.size(),
                    w, f.t0, now_ms());
        const bool chunk_done = f.b.chunk->pending.fetch_sub(1) == 1;
        ring.batch_done();
        // the bases were staged: the arena goes back before the chunk is
        // written (the writer needs only names and CCS)
        if (chunk_done) f.b.chunk->release_arena();
        f.b.chunk.reset();
    };
    // workers whose batches are all finished (the output and the exit wait
    // for this, not for a worker's teardown of its context)
    std::mutex done_m;
    std::condition_variable done_cv;
    int nwork_done = 0;
    auto work_done = [&](int) {
        std::lock_guard<std::mutex> g(done_m);
        ++nwork_done;
        done_cv.notify_all();
    };
    auto worker = [&](int w) {
        if (!async) {
            Flight f;
            while (queue.pop(f.b)) {
                if (fatal) {
                    finish(w, f, -1);
                    continue;
                }
                prepare_in(w, f);
                finish(w, f, ccsx_gpu_run(ctx[w], mode, f.in.data(), f.in.size(), f.out.data()));
            }
            workers_busy.fetch_sub(1);
            work_done(w);
            return;
        }
        // pipelined: up to two batches in flight, the next one submitted
        // before the oldest is collected (include/ccsx_gpu.h).  First the
        // pinned staging of the first slot, sized for a batch (a config-E
        // batch's subreads are ~1/60 of a slot, its tight CCS slabs ~1/3 of
        // that), while step 0 still reads the first chunk
        if (slot_bytes) (void)ccsx_gpu_reserve_staging(ctx[w], slot_bytes / 56, slot_bytes / 160);
        std::deque<Flight> fl;
        for (;;) {
            Flight f;
            const bool got = fl.size() < 2 && (fl.empty() ? queue.pop(f.b) : queue.try_pop(f.b));
            if (got) {
                if (fatal) {
                    finish(w, f, -1);
                    continue;
                }
                prepare_in(w, f);
                const int r = ccsx_gpu_submit(ctx[w], mode, f.in.data(), f.in.size(), &f.slot);
                if (r == -4) {
                    // larger than a slot: collect what is in flight, then
                    // the batch through ccsx_gpu_run's slices
                    while (!fl.empty()) {
                        Flight &g = fl.front();
                        finish(w, g, ccsx_gpu_collect(ctx[w], g.slot, g.out.data()));
                        fl.pop_front();
                    }
                    finish(w, f, ccsx_gpu_run(ctx[w], mode, f.in.data(), f.in.size(), f.out.data()));
                } else if (r != 0) {
                    finish(w, f, r);
                } else {
                    fl.push_back(std::move(f));
                }
                continue;
            }
            if (fl.empty()) break;  // the queue is closed and empty
            Flight &g = fl.front();
            finish(w, g, ccsx_gpu_collect(ctx[w], g.slot, g.out.data()));
            fl.pop_front();
        }
        // a context with no more work releases its pinned staging and device
        // memory while the others run their last batches (≈ 0.2 s each that
        // the process exit would otherwise pay); the last one is left to it.
        // The output waits for the work, not for the release (work_done)
        const bool last = workers_busy.fetch_sub(1) == 1;
        work_done(w);
        if (!fatal && (!last || last_close) && early_close) {
            ccsx_gpu_close(ctx[w]);
            ctx[w] = nullptr;
        }
    };
    std::vector<std::thread> workers;

    // step 0 (main.c:652-697) on its own thread, one chunk ahead of the
    // preparation (the reference's step 0 does both in turn), started before
    // the devices open: HIP's initialisation (~0.1 s) overlaps the first
    // chunk's read.  The reference grows the chunk 1,024 -> 4,096 -> 16,384
    // ZMWs (main.c:686-690); here the sizes scale with the device contexts
    // (known once the devices are counted: until then the first chunk keeps
    // growing; the sizes change only how the work is cut, never the output)
    std::atomic<size_t> chunk_first(SIZE_MAX), chunk_last(SIZE_MAX);
    {
        // the sizes the environment fixes hold from the first record on (the
        // defaults depend on the device count, known once the devices open)
        size_t cm = 0, c0 = 0;
        env_chunk_sizes(0, cm, c0);
        if (cm) chunk_last = cm;
        if (c0) chunk_first = c0;
    }
    ReadQueue rq(1);
    std::thread reader([&]() {
        size_t chunk_size = 0;
        for (size_t id = 0;; ++id) {
            auto ch = std::make_shared<Chunk>();
            ch->id = id;
            ch->pool = &arenas;
            std::vector<Zmw> &zs = ch->zs;
            ch->t_read0 = now_ms();
            ccsx_ingest::ZmwRef zr;
            int l = 0;
            while (!fatal && (l = rd->next(zr)) >= 0) {
                for (const auto &rc : zr.recs) ch->input_hi = std::max(ch->input_hi, rc.seq + rc.span);
                if (l < min_fulllen_count + 2) continue;
                const uint64_t total = zr.total();
                if (total > (uint64_t)max_subread_len || total < (uint64_t)min_subread_len) continue;
                if (have_holes && hole_set.count(zr.hole)) continue;
                zs.emplace_back();
                zs.back().ref = std::move(zr);
                size_t lim = chunk_size ? chunk_size : chunk_first.load();
                if (lim == SIZE_MAX && zs.size() >= kChunkProvisional) {
                    // the devices are still opening: wait for the chunk sizes
                    // rather than grow the first chunk without bound (a slow
                    // HIP init or 16 contexts would put a page-cached input
                    // into one chunk and one arena, with no pipelining)
                    while ((lim = chunk_first.load()) == SIZE_MAX && !fatal)
                        std::this_thread::sleep_for(std::chrono::microseconds(200));
                }
                if (zs.size() >= lim) {
                    chunk_size = std::min(zs.size() * 4, chunk_last.load());
                    break;
                }
            }
            ch->t_read1 = now_ms();
            ch->last_input = l < 0;
            // kt_pipeline stops on an empty chunk (main.c:694-697); a chunk
            // cut short by -1 (end of input or an invalid name) is processed
            // and the next read goes on, as the reference's next step 0 does
            const bool last = zs.empty();
            rq.push(std::move(ch));
            if (last) {
                arenas.drain();
                break;
            }
        }
    });
    // the devices: contexts opened, their workers started (each reserves its
    // first pinned staging at once); a failure ends the process here, before
    // any output
    std::thread opener([&]() {
        auto die = [&](const char *what) {
            fprintf(stderr, "[ccsx] %s\n", what);
            fflush(stderr);
            std::_Exit(1);
        };
        const int ndev = ccsx_gpu_device_count();
        if (ndev <= 0) die("no HIP device: the MI355X engine needs a GPU");
        int ngroup = ndev;
        if (const char *e = getenv("CCSX_NGPU")) ngroup = std::max(1, std::min(64, atoi(e)));
        const int n = ngroup * nslot;
        // the last chunk size: 16,384 ZMWs per pipelined context (one launch
        // per chunk and context), 8,192 per ccsx_gpu_run context (two slices
        // of ~4,096, above the solo configuration's threshold, also with 8
        // GPUs x 2 contexts); the first half of it (the reference starts at
        // 1,024 ZMWs, main.c:686-690, which here only fed small launches on
        // the latency / occupancy objects while the device idled: 62,500
        // config-E ZMWs 6.3 s with 1,024, 5.4 s with 8,192, 5.8 s with 16,384,
        // r04e); CCSX_CHUNK / CCSX_CHUNK0 override
        size_t cmax = 0, c0 = 0;
        env_chunk_sizes(std::min<size_t>((async ? 16384u : 8192u) * (size_t)n, 131072u), cmax, c0);
        chunk_last = cmax;
        chunk_first = c0;  // (the same first size the reader may already be filling to)
        ctx.assign(n, nullptr);
        std::vector<int> per_dev(ndev, 0);
        for (int i = 0; i < n; ++i) per_dev[(i / nslot) % ndev]++;
        for (int i = 0; i < n; ++i) {
            const int dev = (i / nslot) % ndev;
            if (ccsx_gpu_open(dev, &ctx[i]) != 0) die("cannot open a device context");
            ccsx_gpu_set_mem_share(ctx[i], (uint32_t)(per_dev[dev] * dev_share));
            ccsx_gpu_set_prealloc(ctx[i], 1);
            if (verbose > 2 && split_subread) ccsx_gpu_set_bp_log(ctx[i], 1);
            if (fastq) ccsx_gpu_set_quality(ctx[i], 1);
            if (fp_rep) ccsx_gpu_set_pass_stats(ctx[i], 1);
            if (fp_paf || fp_pol) ccsx_gpu_set_base_map(ctx[i], 1);
            if (fp_site) ccsx_gpu_set_pileup(ctx[i], 1);
            if (fp_kin) ccsx_gpu_set_kinetics(ctx[i], 1);
            if (fp_str) ccsx_gpu_set_by_strand(ctx[i], 1);
            if ((kcfg >= 0 && ccsx_gpu_set_kernel_cfg(ctx[i], kcfg) != 0) ||
                (wg_cap > 0 && ccsx_gpu_set_wg_cap(ctx[i], (uint32_t)wg_cap) != 0) ||
                (read_cap > 0 && ccsx_gpu_set_shred_read_cap(ctx[i], (uint32_t)read_cap) != 0) ||
                (mem_frac > 0.f && ccsx_gpu_set_mem_frac(ctx[i], mem_frac) != 0))
                die("invalid CCSX_KCFG / CCSX_WG_PER_CU / CCSX_SHRED_READ_CAP / CCSX_MEM_FRAC");
        }
        if (fp_pol && ccsx_gpu_polish_open(0, 0, &pol) != 0) die("cannot open the polisher context");
        if (bc_path) {
            if (ccsx_gpu_bc_open(0, 0, &bc) != 0) die("cannot open the demultiplexer context");
            if (ccsx_gpu_bc_set(bc, bc_seqs.data(), bc_off.data(), bc_len.data(), (uint32_t)bc_len.size(), (uint32_t)bc_window) != 0)
                die(ccsx_gpu_bc_error(bc));
        }
        if (ad_path) {
            if (ccsx_gpu_scan_open(0, 0, &scn) != 0) die("cannot open the scanner context");
            if (ccsx_gpu_scan_set(scn, ad_seqs.data(), ad_off.data(), ad_len.data(), (uint32_t)ad_len.size(), (uint32_t)ad_min_pct) != 0)
                die(ccsx_gpu_scan_error(scn));
        }
        // pipelined: batches of at most ~95 % of a slot (ccsx_gpu_slot_bytes),
        // so a submitted batch always fits one launch
        if (async && ccsx_gpu_slot_bytes(ctx[0], &slot_bytes) != 0) die(ccsx_gpu_error(ctx[0]));
        if (timing)
            fprintf(stderr, "[ccsx] %d device context(s) open at %.0f ms (main at epoch %.3f s, %.0f ms before)\n", n,
                    now_ms(),
                    std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count() -
                        std::chrono::duration<double>(std::chrono::steady_clock::now() - tmain).count(),
                    std::chrono::duration<double, std::milli>(tstart - tmain).count());
        nctx = n;
        workers_busy = n;
        for (int w = 0; w < n; ++w) workers.emplace_back(worker, w);
    });
    bool opened = false;
    auto await_open = [&]() {
        if (!opened) opener.join();
        opened = true;
    };

    // step 2: ordered output (main.c:707-717)
    size_t nfail = 0;
    size_t nokin = 0;  // -k: lines written without the arrays (a subread lacked ip / pw)
    // the last chunk written stays referenced here and the ones before it are
    // freed on a thread of their own: freeing a chunk (its per-ZMW vectors and
    // strings, the input blocks it holds) takes up to a few hundred ms, which
    // would delay the next chunk's records and, at the end, the exit
    std::shared_ptr<Chunk> last_written;
    ReadQueue reap(1 << 20);
    std::thread reaper([&]() {
        while (auto ch = reap.pop()) ch.reset();
    });
    std::thread writer([&]() {
        while (auto ch = ring.next_done()) {
            if (!fatal && verbose > 2) {
                // main.c:619-620, printed by ccs_for2 during step 1 (so before
                // the chunk's records), to stdout
                for (auto &z : ch->zs)
                    for (size_t r = 0; r + 1 < z.bp.size(); r += 2)
                        fprintf(stdout, "breakpoint=%u maplen=%u nseq=%zu hole=%s\n", z.bp[r], z.bp[r + 1],
                                z.seg_len.size(), z.hole.c_str());
            }
            if (!fatal) {
                for (auto &z : ch->zs) {
                    if (z.status) {
                        ++nfail;
                        fprintf(stderr, "[ccsx] %s/%s: no CCS, the device could not finish this ZMW (%s)\n",
                                z.movie.c_str(), z.hole.c_str(), ccsx_gpu_status_str(z.status));
                        continue;
                    }
                    if (verbose > 1) fprintf(stderr, "poa end %s\n", z.hole.c_str());
                    if (z.ccs.empty()) continue;
                    if (fastq)
                        fprintf(fp_out, "@%s/%s/ccs np=%zu rq=%.6f\n%s\n+\n%s\n", z.movie.c_str(), z.hole.c_str(),
                                z.seg_len.size(), z.rq, z.ccs.c_str(), z.qual.c_str());
                    else
                        fprintf(fp_out, ">%s/%s/ccs\n%s\n", z.movie.c_str(), z.hole.c_str(), z.ccs.c_str());
                    if (fp_rep)
                        for (size_t k = 0; k < z.pst.size(); ++k) {
                            const ccsx_pass_stat &p = z.pst[k];
                            fprintf(fp_rep, "%s/%s/ccs\t%zu\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%.6f\n", z.movie.c_str(),
                                    z.hole.c_str(), k, z.seg_off[k], z.seg_len[k], p.match, p.mismatch, p.ins, p.del, p.cbeg,
                                    p.cend, ccsx_pass_identity(&p));
                        }
                    if (fp_paf) fwrite(z.paf.data(), 1, z.paf.size(), fp_paf);
                    if (fp_site) fwrite(z.sites.data(), 1, z.sites.size(), fp_site);
                    if (fp_str) fwrite(z.strands.data(), 1, z.strands.size(), fp_str);
                    if (fp_pol) fwrite(z.polished.data(), 1, z.polished.size(), fp_pol);
                    if (fp_dmx) fwrite(z.demux.data(), 1, z.demux.size(), fp_dmx);
                    if (fp_bcr) fwrite(z.demux_row.data(), 1, z.demux_row.size(), fp_bcr);
                    if (fp_hit) fwrite(z.scan_rows.data(), 1, z.scan_rows.size(), fp_hit);
                    if (fp_pcs) fwrite(z.pieces.data(), 1, z.pieces.size(), fp_pcs);
                    if (fp_kin) {
                        if (!z.kin_arrays) ++nokin;
                        fwrite(z.kinline.data(), 1, z.kinline.size(), fp_kin);
                    }
                }
            }
            if (timing) fprintf(stderr, "[ccsx] chunk %zu written at %.0f ms\n", ch->id, now_ms());
            if (last_written) reap.push(std::move(last_written));
            last_written = ch;
            ring.pop();
        }
    });

    // the CPU half of step 1: each chunk prepared, cost-ordered and cut into
    // micro-batches for the workers
    for (;;) {
        auto ch = rq.pop();
        if (ch->zs.empty() || fatal) break;
        std::vector<Zmw> &zs = ch->zs;
        const size_t id = ch->id;
        const double t0 = ch->t_read0, t1 = ch->t_read1;
        if (gpu_strand && !aln_tried) {
            // CCSX_GPU_STRAND=1: one aligner context on the first device, opened beside the consensus contexts
            aln_tried = true;
            if (ccsx_gpu_aln_open(0, 0, &aln) != 0) {
                aln = nullptr;
                fprintf(stderr, "[ccsx] CCSX_GPU_STRAND: cannot open the device aligner; preparing on the host\n");
            }
        }
        prepare_chunk(*ch, nthreads, verbose, fp_kin != nullptr, aln, timing);
        // the chunk's bases are in its arena: its input pages go (a mapped
        // file is unmapped behind the reader instead of all at the exit)
        if (input_release) rd->release(ch->input_hi);
        await_open();
        // cost-balanced micro-batches: cost ranks dealt round-robin, each
        // batch longest first (dispatch.cpp)
        const uint32_t n = (uint32_t)zs.size();
        std::vector<uint64_t> cost(n);
        for (uint32_t i = 0; i < n; ++i) cost[i] = ccsx_zmw_cost(zs[i].seg_len.data(), (uint32_t)zs[i].seg_len.size());
        std::vector<uint32_t> order(n), bounds(n + 1);
        uint32_t nparts = (uint32_t)nctx * (ch->last_input ? std::max(batches_per_ctx, last_batches_per_ctx) : batches_per_ctx);
        if (async) {
            uint64_t bytes = 0;
            for (uint32_t i = 0; i < n; ++i) {
                const ccsx_zmw_in zi{zs[i].seqs, zs[i].seg_off.data(), zs[i].seg_len.data(), (uint32_t)zs[i].seg_len.size()};
                bytes += ccsx_gpu_zmw_bytes(ctx[0], mode, &zi);
            }
            const uint64_t per = slot_bytes / 20 * 19;
            nparts = std::max<uint32_t>(nparts, (uint32_t)((bytes + per - 1) / std::max<uint64_t>(per, 1)));
        }
        const uint32_t nb = ccsx_partition(cost.data(), n, nparts, min_batch, order.data(), bounds.data());
        std::vector<Batch> bs(nb);
        for (uint32_t b = 0; b < nb; ++b) {
            bs[b].chunk = ch;
            bs[b].idx.assign(order.begin() + bounds[b], order.begin() + bounds[b + 1]);
        }
        ch->pending = nb;
        if (timing)
            fprintf(stderr, "[ccsx] chunk %zu: %u ZMWs read %.0f-%.0f ms, prepared until %.0f ms, %u batches\n", id, n,
                    t0, t1, now_ms(), nb);
        ring.add(ch);  // blocks while 3 chunks are ahead of the writer
        queue.push(std::move(bs));
    }
    // at the end of the input the reader has pushed its empty chunk and
    // returned; after a fatal device error it stops at its next record and
    // pushes without waiting for space
    await_open();
    rq.stop();
    reader.join();
    ring.finish();
    queue.close();
    {
        std::unique_lock<std::mutex> g(done_m);
        done_cv.wait(g, [&] { return nwork_done == nctx; });
    }
    if (fatal) ring.stop();
    writer.join();
    const double tw = now_ms();
    if (!fatal) {
        // (a worker may still be releasing its context: the exit ends it)
        // every byte is written: flush and leave without tearing down the
        // device contexts (≈ 0.8 s of hipFree / hipHostFree for a 100k run)
        // or the last chunk; process exit releases both
        // a failed final write (ENOSPC, EPIPE on a FIFO) must not exit 0
        bool werr = fp_out != stdout && (ferror(fp_out) || fclose(fp_out) != 0);
        if (fp_rep) werr = (ferror(fp_rep) || fclose(fp_rep) != 0) || werr;
        if (fp_paf) werr = (ferror(fp_paf) || fclose(fp_paf) != 0) || werr;
        if (fp_site) werr = (ferror(fp_site) || fclose(fp_site) != 0) || werr;
        if (fp_kin) werr = (ferror(fp_kin) || fclose(fp_kin) != 0) || werr;
        if (fp_str) werr = (ferror(fp_str) || fclose(fp_str) != 0) || werr;
        if (fp_pol) werr = (ferror(fp_pol) || fclose(fp_pol) != 0) || werr;
        if (fp_dmx) werr = (ferror(fp_dmx) || fclose(fp_dmx) != 0) || werr;
        if (fp_bcr) werr = (ferror(fp_bcr) || fclose(fp_bcr) != 0) || werr;
        if (fp_hit) werr = (ferror(fp_hit) || fclose(fp_hit) != 0) || werr;
        if (fp_pcs) werr = (ferror(fp_pcs) || fclose(fp_pcs) != 0) || werr;
        werr = (ferror(stdout) || fflush(stdout) != 0) || werr;  // (-v >= 3 breakpoint lines go to stdout)
        if (werr) fprintf(stderr, "[ccsx] error writing the output: %s\n", strerror(errno));
        if (getenv("CCSX_EXIT_CLOSE")) {  // measurement: the teardown steps the exit skips, timed
            const double a = now_ms();
            for (auto &t : workers) t.join();
            for (auto *x : ctx) ccsx_gpu_close(x);
            const double b = now_ms();
            rd.reset();
            const double d = now_ms();
            reap.push(nullptr);
            reaper.join();
            last_written.reset();
            std::string mem;
            if (FILE *f = fopen("/proc/self/smaps_rollup", "r")) {
                char ln[256];
                while (fgets(ln, sizeof ln, f))
                    if (!strncmp(ln, "AnonHugePages", 13) || !strncmp(ln, "Rss", 3) || !strncmp(ln, "Anonymous", 9))
                        mem += std::string(ln, strcspn(ln, "\n")) + "; ";
                fclose(f);
            }
            fprintf(stderr, "[ccsx] teardown: contexts %.0f ms, input %.0f ms, last chunk %.0f ms (then %s)\n", b - a,
                    d - b, now_ms() - d, mem.c_str());
        }
        if (timing)
            fprintf(stderr, "[ccsx] output done at %.0f ms; device cells %llu; exit at epoch %.3f s\n", tw,
                    (unsigned long long)cells_total.load(),
                    std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count());
        if (nfail) fprintf(stderr, "[ccsx] %zu ZMWs had no CCS (device status, see above)\n", nfail);
        if (fp_kin) fprintf(stderr, "[ccsx] %zu ZMWs without kinetics: their -k lines carry no fi/fp/ri/rp arrays\n", nokin);
        fflush(stderr);
        std::_Exit(werr ? 1 : 0);
    }
    for (auto &t : workers) t.join();
    for (auto *x : ctx) ccsx_gpu_close(x);
    ccsx_gpu_aln_close(aln);
    ccsx_gpu_polish_close(pol);
    ccsx_gpu_bc_close(bc);
    ccsx_gpu_scan_close(scn);
    reap.push(nullptr);
    reaper.join();
    if (timing) fprintf(stderr, "[ccsx] output done at %.0f ms, contexts closed at %.0f ms\n", tw, now_ms());
    rd.reset();
    if (fp_out != stdout) (void)fclose(fp_out);
    else (void)fflush(stdout);
    if (fp_rep) (void)fclose(fp_rep);
    if (fp_paf) (void)fclose(fp_paf);
    if (fp_site) (void)fclose(fp_site);
    if (fp_kin) (void)fclose(fp_kin);
    if (fp_str) (void)fclose(fp_str);
    if (fp_pol) (void)fclose(fp_pol);
    if (fp_dmx) (void)fclose(fp_dmx);
    if (fp_bcr) (void)fclose(fp_bcr);
    if (fp_hit) (void)fclose(fp_hit);
    if (fp_pcs) (void)fclose(fp_pcs);
    if (nfail) fprintf(stderr, "[ccsx] %zu ZMWs had no CCS (device status, see above)\n", nfail);
    return fatal ? 1 : 0;
}
