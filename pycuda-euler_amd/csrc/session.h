// session.h -- the host side of a session: its device / pinned buffers, ec_session itself, the
// resets of its device-backed state and the small device -> host reads; then what the count phases
// (count_phase.h) and the graph phase (assemble.hip) both stand on: the device scalars block, the
// rocprim scan / sort wrappers, the host-input pipeline's pipe_upto, the timing marks,
// compact_table and the shared checks.  Included by assemble.hip after the kernel headers whose
// types the session holds (SolidIndex, XAlpha, SuperRec).
//
// A device buffer of a session exists only through EC_SESSION_BUFS below: the list expands to the
// DevBuf members and to for_each_buf, so what ec_session_bytes counts, ec_session_trim releases
// and the destructor frees is by construction every buffer there is.
#pragma once
#include "common.h"
#include "compact.h"
#include "graph.h"
#include "hostin.h"

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <dlfcn.h>
#include <utility>
#include <vector>

namespace ec {

// device bytes the process's session buffers hold, and their high-water mark (ec_mem_stats:
// the per-rank HBM of the sharded and streaming paths is reported from these)
inline std::atomic<unsigned long long> g_hbm_held{0}, g_hbm_peak{0};
inline void hbm_account(long long d) {
    const unsigned long long now = g_hbm_held.fetch_add((unsigned long long)d) + (unsigned long long)d;
    unsigned long long pk = g_hbm_peak.load();
    while (now > pk && !g_hbm_peak.compare_exchange_weak(pk, now)) {
    }
}
bool memlog_on();

// device buffer: owns its allocation (freed with the buffer), moves but does not copy
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        std::swap(p, o.p);
        std::swap(cap, o.cap);
        return *this;
    }
    ~DevBuf() { release(); }
    // (spare: allocate that fraction more already the first time -- a size that varies from call
    // to call, like the gathered chain count)
    __attribute__((noinline)) int ensure(size_t bytes, unsigned int spare_div = 0) {
        if (bytes <= cap) return EC_OK;
        // a buffer that grows gets 1/8 of headroom: sizes that vary a little from call to call
        // (chain counts, received records) would otherwise reallocate -- ~1 ms a hipFree /
        // hipMalloc pair -- on every call that is a little larger than the last
        size_t want = std::max<size_t>(bytes, 256);
        if (cap) want += want / 8;
        else if (spare_div) want += want / spare_div;
        release();
        const auto t0 = std::chrono::steady_clock::now();
        if (hipMalloc(&p, want) != hipSuccess) {
            p = nullptr;
            set_error("hipMalloc(%zu) failed", want);
            return EC_ERR_NOMEM;
        }
        cap = want;
        hbm_account((long long)want);
        if (want >= (1ull << 30) && memlog_on()) {  // EULERHIP_MEMLOG=1: large buffers and their call sites
            // (lib+offset: llvm-symbolizer --obj=libeulerhip.so of the same build names the caller)
            Dl_info di{};
            void *ra = __builtin_return_address(0);
            const unsigned long off = dladdr(ra, &di) && di.dli_fbase ? (unsigned long)((char *)ra - (char *)di.dli_fbase) : 0ul;
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            fprintf(stderr, "[eulerhip mem] +%.2f GB (held %.2f GB) in %.1f ms at lib+0x%lx\n", want / 1e9,
                    g_hbm_held.load() / 1e9, ms, off);
        }
        return EC_OK;
    }
    template <typename T>
    T *as() const { return reinterpret_cast<T *>(p); }
    void release() {
        if (p) {
            const auto t0 = std::chrono::steady_clock::now();
            hipFree(p);
            hbm_account(-(long long)cap);
            if (cap >= (1ull << 30) && memlog_on())
                fprintf(stderr, "[eulerhip mem] -%.2f GB (held %.2f GB) in %.1f ms\n", cap / 1e9, g_hbm_held.load() / 1e9,
                        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        }
        p = nullptr;
        cap = 0;
    }
};

// pinned host buffer (page-locked: D2H copies of the results run at full PCIe rate)
struct HostBuf {
    char *p = nullptr;
    size_t cap = 0, size = 0;
    HostBuf() = default;
    HostBuf(const HostBuf &) = delete;
    HostBuf &operator=(const HostBuf &) = delete;
    ~HostBuf() { release(); }
    int resize(size_t bytes) {
        size = bytes;
        if (bytes <= cap) return EC_OK;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        size_t want = std::max<size_t>(bytes + bytes / 4, 4096);
        if (hipHostMalloc(reinterpret_cast<void **>(&p), want, hipHostMallocDefault) != hipSuccess) {
            p = nullptr;
            size = 0;
            set_error("hipHostMalloc(%zu) failed", want);
            return EC_ERR_NOMEM;
        }
        cap = want;
        return EC_OK;
    }
    char *data() const { return p; }
    bool empty() const { return size == 0; }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = size = 0;
    }
};

template <typename T>
struct PinnedVec {  // std::vector-like view of a pinned HostBuf
    HostBuf b;
    size_t n = 0;
    PinnedVec() = default;
    PinnedVec(const PinnedVec &) = delete;
    PinnedVec &operator=(const PinnedVec &) = delete;
    ~PinnedVec() { release(); }
    int resize(size_t count) {
        n = count;
        return b.resize(count * sizeof(T));
    }
    T *data() const { return reinterpret_cast<T *>(b.p); }
    size_t size() const { return n; }
    bool empty() const { return n == 0; }
    T &operator[](size_t i) const { return data()[i]; }
    void release() {
        b.release();
        n = 0;
    }
};

}  // namespace ec

using namespace ec;

// Every device buffer of a session, grouped by the phase that owns it (several are reused by a
// later phase while their owner's data is dead; the call sites say so).  X(name) per buffer.
#define EC_SESSION_BUFS(X)                                                                                          \
    /* count: HyperLogLog, the scalars block, hash table, the dense solid arrays (key, count, first events),     \
       partition histograms / cursors / records, compaction and scan scratch (rbc, tmp), the owner merge's ids */  \
    X(hll) X(scal) X(table) X(dkey) X(dcnt) X(dfc) X(dft)                                                           \
    X(hist) X(ftot) X(cnt) X(offs) X(bstart) X(tot) X(recs) X(recs2) X(sub) X(ocnt) X(rbc) X(tmp)                   \
    X(mbid) X(mbid2) X(midx) X(midx2) X(gcur)                                                                       \
    /* ... k_bucket_filt's per-bucket part bits; count_v2.h final-bucket cursors, bucket bounds; k_skdedup's      \
       merged records of the error-rich count; bmark: bucket starts of the dense ids (k_skbucket3 marks each      \
       bucket's first id), where the tile ranking cuts its tiles (k_tile_plan) */                                  \
    X(bnp) X(fcur) X(bb2) X(skm_rec) X(skm_ev) X(skm_end) X(bmark)                                                  \
    /* wide count (count_wide.h, k > 32): every window's minimizer, k_wbv's 2-bit copy of the reads (config 5's   \
       run codes gathered from it), k_run_codes' first code dword of each third-level table */                     \
    X(wbv) X(rpack) X(wcodes_tab)                                                                                   \
    /* graph links: palindrome flags, out-degrees, candidates, succ / pred, graph.h NodeRec (successor + first     \
       event per node, k_walk); join_local.h per-key table words, table id ranges, foreign counts / offsets,      \
       flags, and the speculated prologue's foreign records (s->recs still feeds a second refine) */               \
    X(upal) X(outdeg) X(cand) X(succ) X(pred) X(nrec)                                                               \
    X(jl_kof) X(jl_rs) X(jl_re) X(jl_cnt) X(jl_off) X(jl_flag) X(jl_frec)                                           \
    /* ranking: ruling set + Wyllie state, path key / rank / length / min; rank_tile.h tile bounds, counts /       \
       bases, super list, its walk records, index map, path keys / ranks, k_tile_chains' look-back words */        \
    X(st0) X(st1) X(rid) X(rlist) X(nextR) X(PK) X(RK) X(PL) X(PM)                                                  \
    X(rt_tb) X(rt_tcnt) X(rt_tbase) X(rt_srec) X(rt_snrec) X(rt_sidx) X(rt_pks) X(rt_rks) X(rt_hasp) X(rt_lr)       \
    X(rt_lb)                                                                                                        \
    /* starts / emit / GFA: start keys and nodes (sorted), contig index / lengths / offsets / characters / end     \
       nodes, walks, link table and counts, the results' transfer forms (dchars, dcounts, lc8; dchars / dcounts   \
       are also ec_assemble_kmers' input) */                                                                       \
    X(skeys) X(svals) X(skeys2) X(svals2) X(cidxOf) X(clen) X(coff) X(chars) X(cfirst) X(clast) X(headOf)           \
    X(tailOf) X(cwalk) X(ewalk) X(lk) X(lcnt) X(lc8) X(dchars) X(dcounts)                                           \
    /* stepwise / junction (junction.h): record / outbox scratch of the distributed join, ec_merge_owned_from's    \
       decoded records, the partitioned finish's transfer record (chunk counts and scans, end records) */          \
    X(jrec) X(joid) X(jout) X(jseg) X(jcnt) X(xrec) X(run_cnt) X(run_ends) X(run_dends)                             \
    /* extended alphabet (extended.h): the one-way-link components' union-find / cut / emulation buffers */        \
    X(x_par) X(x_irr) X(x_in) X(x_succ) X(x_done) X(x_lk) X(x_lv) X(x_lk2) X(x_lv2) X(x_len) X(x_m) X(x_cid)        \
    X(x_head) X(x_tail)                                                                                             \
    /* clip / pop / spectrum (clip.h, pop.h, spectrum.h): tip candidates, lists, kills, totals; branch keys,       \
       per-contig sums, the tile table; the global histogram */                                                    \
    X(clip_cand) X(clip_list) X(clip_kill) X(clip_tot) X(pop_key) X(pop_sum) X(pop_tcnt) X(pop_toff) X(pop_tile)    \
    X(spec_hist)                                                                                                    \
    /* host input: H2D staging of ec_assemble_host, the unstaged packed input's codes and exceptions */            \
    X(h_reads) X(h_offsets) X(p_codes) X(p_exc)

struct ec_session {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
#define EC_BUF_MEMBER(name) DevBuf name;
    EC_SESSION_BUFS(EC_BUF_MEMBER)
#undef EC_BUF_MEMBER
    // results (host)
    bool have = false;
    int k = 0;
    ec_stats stats{};
    HostBuf h_chars;
    // the one-GPU results' characters in transfer form: 2-bit codes, 4 a byte (A C G T = 0..3;
    // every character of a standard-alphabet contig is one of them), nchars_host of them --
    // ec_copy_contigs widens them (ecoli10m_err: 38 MB of characters over PCIe took ~0.7 ms)
    bool chars_packed = false;
    uint64_t nchars_host = 0;
    // small device -> host reads (scalars, counts) go through this page-locked bounce buffer and
    // are delivered by host_sync: a pageable destination cost ~11 us more per round trip
    // (tools/micro/sync_lat.hip on MI355X: 27.2 vs 16.3 us), and a step has ~6 of them
    HostBuf bounce;
    struct Pend {
        void *dst;
        size_t off, n;
    };
    std::vector<Pend> pend;
    size_t bused = 0;
    hipEvent_t rd_ev = nullptr;  // host_wait: a read-back's event (created on first use)
    // the contig characters' early copy to host memory (phase_graph): its stream and events, and
    // the previous call's character total that sizes it
    hipStream_t ostream = nullptr;
    // oev[0] / [1]: emission done / characters copied; [2] contig offsets final; [3] link offsets final
    hipEvent_t oev[4] = {nullptr, nullptr, nullptr, nullptr};
    uint64_t last_nchars = 0;
    // bmark (the dense ids' bucket starts) is valid from a super-k-mer count to its graph phase
    bool bmark_ok = false;
    // the owner merge's marks (phase_merge_part): its solid count, 0 = none -- the partitioned
    // finish cuts its segment's tiles there when the segment is that merge's output
    uint64_t seg_marks = 0;
    // count_sk2's refine plan of the previous call: launched speculatively on the next call of
    // the same shape while the host reads the partition's scalars back (phase_count_sk2)
    struct SkSpec {
        bool valid = false;
        uint64_t G = 0, cap = 0, nreads = 0, read_base = 0, fcap = 0;
        uint32_t M = 0;
        int k = 0, bbits = 0;
    } skspec;
    // links_local's first two kernels (k_jl_init, k_jl_scan) queued by phase_count_sk2 behind its
    // bucket kernel, on the previous call's shape, while the host waits for the solid count: the
    // scan reads U from the device and stops at ucap.  valid: links_local's shape of the previous
    // call; queued: this call's prologue is in the stream and the count has not been redone since.
    // Odd k only (even k needs k_upal between the two; left unspeculated)
    struct JlSpec {
        bool valid = false, queued = false;
        int bits = 0, k = 0;
        unsigned int ucap = 0, fcap = 0;
    } jlspec;
    bool graph_follows = false;  // the call goes on to phase_graph (assemble): the prologue may run
    // ec_spec_counts: prologues kept / run again behind the solid count's read-back [0], [1]; the
    // same for the contig starts' read-back [2], [3], on which nothing is queued
    uint64_t spec_cnt[4] = {0, 0, 0, 0};
    PinnedVec<uint64_t> h_coff;  // result readbacks land in pinned host memory
    PinnedVec<uint64_t> h_loff;
    PinnedVec<int64_t> h_links;
    // the one-GPU results' links in transfer form (links_compact): per-side link counts as bytes
    // and the links as u32 (2 contig + end < 2^32) -- ec_copy_links widens them (ecoli10m_err:
    // 18 + 18 MB of u64 offsets and links after GFA cost ~0.65 ms of PCIe; now 2.2 + 9 MB)
    PinnedVec<uint8_t> h_lc8;
    PinnedVec<uint32_t> h_links32;
    bool links_compact = false;
    // few contigs (k_links_small): link total, emission flag, contig offsets, links and link counts
    // as one block (in dcounts on the device), copied once and taken apart on the host
    HostBuf h_blk;
    bool want_dict = false;
    hipEvent_t ev[2 * EC_NSTAGES] = {};
    hipEvent_t kev[2 * EC_NKERNELS] = {};
    bool kused[EC_NKERNELS] = {};
    bool sused[EC_NSTAGES] = {};
    bool events = false;
    bool timing = false;        // kernel events (EC_FLAG_TIMING or EC_FLAG_KERNEL_TIMING)
    bool stage_timing = false;  // stage events (EC_FLAG_TIMING)
    unsigned int n_dense = 0;  // dense k-mer arrays held by the session (shard / merge steps)
    bool dense_ok = false;     // ... as ec_count_shard / ec_merge_owned left them (ec_export_* valid)
    bool stats_ok = false;     // ec_get_stats valid (any successful call)
    unsigned flags = 0;        // flags of the current call
    bool no_index = false;      // the call needs dense records only (shard count, owner merge)
    uint64_t shard_base = 0;    // ec_count_shard: global id of the shard's read 0 (added at export)
    // the super-k-mer fast path's read length of the last call on (offsets, reads): reused
    // without a host round trip -- k_skpart_w<., ., true> checks every read against it anyway
    const uint64_t *lc_off = nullptr;
    uint64_t lc_n = 0, lc_L = 0;
    SolidIndex gidx{};          // index of the loaded solid set (ec_graph_load, k <= 32)
    SolidIndexW gidxw{};        // the same for k > 32
    bool graph_loaded = false;  // ec_graph_load held: ec_graph_links_part / ec_graph_finish valid
    // junction-partitioned graph (junction.h, round 5): the segment placed at its global ids
    // (ec_graph_place), no global set held
    bool placed = false;
    uint64_t seg_lo = 0, seg_Ur = 0;
    HostBuf hmeta;   // ec_merge_owned_from: the received records' per-source table, staged page-locked
    int owner_rule = 0;         // ec_session_set_owner_rule: 0 minimizer ranges (21 <= k <= 52), 1 key hash
    // ec_export_by_owner's owner ids / scanned chunk histogram of the last call, reused by a
    // following call with the same records, owners and rule (counts first, then the scatter)
    bool own_valid = false;
    int own_rule = 0, own_nowners = 0;
    unsigned int own_n = 0, own_nblk = 0;
    std::vector<unsigned int> own_hi;
    // host-input pipeline (ec_assemble_host / ec_assemble_packed_host, hostin.h): the reads are
    // copied H2D in chunks on cstream; pipe_upto(c) makes chunks .. c visible to the session
    // stream (event wait + unpack) -- the super-k-mer partition runs on each chunk's read groups
    // as they arrive, any other count path waits for all of them (pipe_all)
    // (one copy stream: an SDMA copy runs at half its idle rate while the count kernels run
    // (r06_i trace), and chunks alternating over two queues did not help -- pipelined 5.22 /
    // 5.22 ms on one, 5.23 / 5.95 on two: r06_m)
    hipStream_t cstream = nullptr;
    struct Pipe {
        bool active = false;
        bool packed = false;          // 2-bit codes (k_unpack2 + k_patch) or ASCII
        int nchunks = 0, done = 0;    // chunks made visible so far
        std::vector<uint64_t> blo, bhi;   // chunk c = bases [blo[c], bhi[c]) (multiples of 64 inside)
        std::vector<uint64_t> ravail;     // reads complete after chunk c
        std::vector<uint64_t> elo, ehi;   // its exceptions (packed)
        uint64_t first_len = 0;           // length of read 0 (the partition's M before any D2H)
        const uint32_t *codes = nullptr;  // device 2-bit codes
        const uint64_t *exc_pos = nullptr;
        const uint8_t *exc_byte = nullptr;
        uint8_t *ascii = nullptr;         // device reads (the count kernels' input)
        std::vector<hipEvent_t> ev;       // chunk copy events (created on demand, reused)
    } pipe;
    // staged packed batches (ec_stage_packed_host / ec_assemble_staged): two slots, so the copy
    // of batch i + 1 runs on cstream while batch i is assembled; free_ev = the slot's last
    // reader (its assemble call) done on the session stream
    struct Staged {
        Pipe pipe;
        // the only device buffers outside EC_SESSION_BUFS: a staged batch outlives a trim and is
        // not counted by ec_session_bytes (include/eulerhip.h); freed with the session
        DevBuf codes, exc, off;
        hipEvent_t free_ev = nullptr;
        uint64_t nreads = 0, nbases = 0;
    } stg[2];
    int stg_head = 0, stg_n = 0;
    // extended alphabet (extended.h): its symbol table
    bool xalpha = false;
    XAlpha xa{};
    // Wyllie rounds the last converged super ranking needed + 1 (0: none yet, or it did not
    // converge): rank_supers_async queues that many instead of ceil(log2 N) + 2 -- a round after
    // convergence still costs its launch (~5 us; the headline needs ~18 of 26) -- and a shortfall
    // is caught by the convergence check that already follows (the ranking redone, host-checked)
    int spec_rounds = 0;
    // multi-GPU partitioned finish (ec_graph_chains_part ..): this rank's segment of oriented nodes
    uint64_t seg_n0 = 0, seg_n1 = 0;
    // a partitioned step called with a NULL output (ec_graph_place / chains_part / starts_part):
    // its records counted and held here until the matching ec_graph_*_copy writes them into a
    // buffer of the exact size (1: junction records, 2: super records, 3: start records)
    struct Pending {
        int kind = 0;
        uint64_t n = 0;
        unsigned int ntiles = 0;
        bool planned = false;
    } hold;
    SuperRec *chain_scr = nullptr;  // part_chains' tile records (st1, or a placed segment's jrec)
    unsigned int seg_nc = 0;     // contigs of the job (ec_graph_layout)
    uint64_t seg_nchars = 0;
    // the partitioned finish's transfer record (ec_graph_emit_runs / ec_graph_copy_runs): its sizes
    unsigned long long lb_epoch = 0;  // rt_lb's current epoch (rank_tile.h TileLB)
    uint64_t run_nr = 0, run_nch = 0, run_nends = 0;
    bool runs_ready = false;
    // how far the partitioned finish of the loaded / placed set has come: each step needs the one
    // before it (0 none, 1 chains, 2 super ranking, 3 starts, 4 layout, 5 emitted)
    int part_stage = 0;
    // ec_clip_tips (clip.h): valid only on the results of a one-GPU graph phase whose dense arrays,
    // lookup index, contig characters / offsets and link table are still on the device.  clip_ok is
    // set where such a phase ends and cleared by everything that rewrites or releases them
    // (drop_device_state); clip_why says what the refusal reports.  cidx / cidxw: the index the
    // count or merge returned, kept past the call (as gidx / gidxw keep a loaded set's)
    bool clip_ok = false;
    const char *clip_why = "a new session holds no assembly";
    SolidIndex cidx{};
    SolidIndexW cidxw{};
};

// every device buffer of a session (bytes, trim)
template <typename Fn>
static void for_each_buf(ec_session *s, Fn fn) {
#define EC_BUF_VISIT(name) fn(s->name);
    EC_SESSION_BUFS(EC_BUF_VISIT)
#undef EC_BUF_VISIT
}

// ec_clip_tips' refusal after the stepwise calls (ec_session::clip_why)
static const char *const CLIP_WHY_STEPWISE =
    "the last calls were stepwise ones (ec_count_shard / ec_merge_owned* / ec_graph_*), which leave no one-GPU assembly";

// Every piece of step state that points into session buffers: records held for an ec_graph_*_copy,
// the emitted runs, the chain records' scratch, the partitioned finish's progress.  Dropped by
// whatever releases, rewrites or may reallocate those buffers (trim, a new call, a new load /
// place / join), so a late copy or step is refused instead of reading them (include/eulerhip.h).
static inline void drop_step_state(ec_session *s) {
    s->hold.kind = 0;
    s->runs_ready = false;
    s->chain_scr = nullptr;
    s->part_stage = 0;
}

// Everything the session knows about what its device buffers hold, dropped by what rewrites them
// all (begin_call) or releases them (ec_session_trim): the step state, a loaded / placed graph,
// the dense arrays, the one-GPU assembly ec_clip_tips reads (why: what its refusal reports), the
// export's owner ids and the tile marks.  The narrower resets (ec_graph_load, graph_place,
// ec_dense_refilter) keep part of it on purpose.
static inline void drop_device_state(ec_session *s, const char *why) {
    drop_step_state(s);
    s->graph_loaded = false;
    s->placed = false;
    s->dense_ok = false;
    s->clip_ok = false;
    s->clip_why = why;
    s->own_valid = false;
    s->bmark_ok = false;
    s->seg_marks = 0;
}

namespace {
constexpr size_t BOUNCE_CAP = 64 << 10, BOUNCE_MAX = 16 << 10;  // bytes; larger reads go direct

// queue a device -> host copy of n bytes to dst on st; dst is valid after host_sync(s, st)
inline int d2h(ec_session *s, void *dst, const void *src, size_t n, hipStream_t st) {
    if (!n) return EC_OK;
    const size_t off = (s->bused + 15) & ~size_t(15);
    if (n > BOUNCE_MAX || off + n > BOUNCE_CAP) {
        EC_HIP(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, st));
        return EC_OK;
    }
    if (!s->bounce.p) EC_CHECK(s->bounce.resize(BOUNCE_CAP));
    EC_HIP(hipMemcpyAsync(s->bounce.p + off, src, n, hipMemcpyDeviceToHost, st));
    s->pend.push_back({dst, off, n});
    s->bused = off + n;
    return EC_OK;
}

// wait for event ev (recorded after the d2h copies), then deliver the queued d2h reads: the
// stream may run on past it
inline int host_wait(ec_session *s, hipEvent_t ev) {
    const hipError_t e = hipEventSynchronize(ev);
    for (const auto &q : s->pend) std::memcpy(q.dst, s->bounce.p + q.off, q.n);
    s->pend.clear();
    s->bused = 0;
    if (e != hipSuccess) {
        set_error("HIP error %s", hipGetErrorString(e));
        return EC_ERR_HIP;
    }
    return EC_OK;
}

// wait for st, then deliver the queued d2h reads
inline int host_sync(ec_session *s, hipStream_t st) {
    const hipError_t e = hipStreamSynchronize(st);
    for (const auto &q : s->pend) std::memcpy(q.dst, s->bounce.p + q.off, q.n);
    s->pend.clear();
    s->bused = 0;
    if (e != hipSuccess) {
        set_error("HIP error %s", hipGetErrorString(e));
        return EC_ERR_HIP;
    }
    return EC_OK;
}

struct Scalars {  // device scalars block
    unsigned long long npos;
    unsigned long long bad;
    unsigned long long ndistinct;
    double est;
    unsigned int overflow;
    unsigned int nsolid;
    unsigned int nstarts;
    unsigned int final_sel;
    unsigned int ndict;
    unsigned int nr;
    unsigned int npal;
    unsigned int ngath;  // phase_load_det: non-filler records of a gathered solid set
    unsigned long long nvisited;
    unsigned int maxlocal;
    unsigned int skew;
    unsigned int lens[4];  // k_upsweep: max read length, ~min read length (reads with windows), any slow-path read
    unsigned long long nrec;  // k_upsweep_sk: super-k-mer records
    unsigned int nasym, nxl, nxs;  // extended.h: one-way links, entries of their components, their starts
    unsigned int xbad;             // extended.h: a walk that never reaches its start again
    unsigned int wbv_long, wpad;     // k_wbv: a read of another length
    unsigned long long chains;       // k_tile_compact: the tile contraction's chain count
    unsigned int active[64];
};
static_assert(sizeof(Scalars) % 8 == 0 && offsetof(Scalars, bad) % 8 == 0, "k_scal_reset writes 64-bit words");

// the scalars as a call finds them, in one launch (two fills before): all zero, bad = ~0
__global__ void __launch_bounds__(64) k_scal_reset(Scalars *sc) {
    unsigned long long *w = reinterpret_cast<unsigned long long *>(sc);
    for (unsigned int i = threadIdx.x; i < sizeof(Scalars) / 8; i += 64)
        w[i] = i == offsetof(Scalars, bad) / 8 ? ~0ull : 0ull;
}

int scan_u64(ec_session *s, const unsigned long long *in, unsigned long long *out, size_t n) {
    size_t bytes = 0;
    EC_HIP(rocprim::exclusive_scan(nullptr, bytes, in, out, 0ull, n, rocprim::plus<unsigned long long>(), s->stream));
    EC_CHECK(s->tmp.ensure(bytes));
    EC_HIP(rocprim::exclusive_scan(s->tmp.p, bytes, in, out, 0ull, n, rocprim::plus<unsigned long long>(), s->stream));
    return EC_OK;
}

int scan_excl_u32(ec_session *s, const unsigned int *in, unsigned int *out, size_t n) {
    size_t bytes = 0;
    EC_HIP(rocprim::exclusive_scan(nullptr, bytes, in, out, 0u, n, rocprim::plus<unsigned int>(), s->stream));
    EC_CHECK(s->tmp.ensure(bytes));
    EC_HIP(rocprim::exclusive_scan(s->tmp.p, bytes, in, out, 0u, n, rocprim::plus<unsigned int>(), s->stream));
    return EC_OK;
}

int scan_incl_u32(ec_session *s, const unsigned int *in, unsigned int *out, size_t n) {
    size_t bytes = 0;
    EC_HIP(rocprim::inclusive_scan(nullptr, bytes, in, out, n, rocprim::plus<unsigned int>(), s->stream));
    EC_CHECK(s->tmp.ensure(bytes));
    EC_HIP(rocprim::inclusive_scan(s->tmp.p, bytes, in, out, n, rocprim::plus<unsigned int>(), s->stream));
    return EC_OK;
}

int sort_pairs(ec_session *s, unsigned long long *kin, unsigned long long *kout, unsigned int *vin, unsigned int *vout,
               size_t n) {
    size_t bytes = 0;
    EC_HIP(rocprim::radix_sort_pairs(nullptr, bytes, kin, kout, vin, vout, n, 0, 64, s->stream));
    EC_CHECK(s->tmp.ensure(bytes));
    EC_HIP(rocprim::radix_sort_pairs(s->tmp.p, bytes, kin, kout, vin, vout, n, 0, 64, s->stream));
    return EC_OK;
}

// make host-input chunks .. c visible on the session stream (no-op without a pipeline)
int pipe_upto(ec_session *s, int c) {
    auto &pp = s->pipe;
    if (!pp.active) return EC_OK;
    c = std::min(c, pp.nchunks - 1);
    if (pp.done > c) return EC_OK;
    const int first = pp.done;
    for (; pp.done <= c; pp.done++) EC_HIP(hipStreamWaitEvent(s->stream, pp.ev[pp.done], 0));
    // one unpack over the chunks made visible together (their ranges are contiguous)
    const uint64_t blo = pp.blo[first], bhi = pp.bhi[c], elo = pp.elo[first], ehi = pp.ehi[c];
    if (pp.packed && bhi > blo) {
        const uint64_t units = ((bhi + 15) >> 4) - (blo >> 4);
        k_unpack2<<<grid_for(units, 256, 16384), 256, 0, s->stream>>>(pp.codes, blo, bhi, pp.ascii);
        if (ehi > elo)
            k_patch<<<grid_for(ehi - elo, 256, 4096), 256, 0, s->stream>>>(pp.exc_pos, pp.exc_byte, elo, ehi,
                                                                           pp.ascii);
    }
    return EC_OK;
}
int pipe_all(ec_session *s) { return s->pipe.active ? pipe_upto(s, s->pipe.nchunks - 1) : EC_OK; }

inline void mark(ec_session *s, int idx) {
    if (s->stage_timing) {
        hipEventRecord(s->ev[idx], s->stream);
        if (idx & 1) s->sused[idx >> 1] = true;
    }
}
// kernel-level timing events: kernel id, 0 = before / 1 = after
inline void kmark(ec_session *s, int kid, int end) {
    if (s->timing) {
        hipEventRecord(s->kev[2 * kid + end], s->stream);
        if (end) s->kused[kid] = true;
    }
}

// solid slots of an HBM table -> dense arrays (ids in table order); sets dsc->nsolid / ndistinct
template <typename SlotT, typename KeyT>
int compact_table(ec_session *s, SlotT *table, uint64_t cap, long long limit, KeyT *dkey) {
    hipStream_t st = s->stream;
    Scalars *dsc = s->scal.as<Scalars>();
    const unsigned int nblk = (unsigned int)((cap + COMPACT_CHUNK - 1) / COMPACT_CHUNK);
    EC_CHECK(s->rbc.ensure((size_t)nblk * 8 + 8));
    unsigned int *bc = s->rbc.as<unsigned int>(), *bs = bc + nblk;
    EC_HIP(hipMemsetAsync(&dsc->nsolid, 0, 4, st));
    EC_HIP(hipMemsetAsync(&dsc->ndistinct, 0, 8, st));
    k_compact_count<SlotT><<<nblk, 256, 0, st>>>(table, cap, limit, bc, &dsc->ndistinct);
    EC_CHECK(scan_incl_u32(s, bc, bs, nblk));
    k_compact_write<SlotT, KeyT><<<nblk, 256, 0, st>>>(table, cap, limit, bs, dkey, s->dcnt.as<unsigned int>(),
                                                      s->dfc.as<unsigned long long>(),
                                                      s->dft.as<unsigned long long>());
    k_compact_total<<<1, 1, 0, st>>>(bs, nblk, &dsc->nsolid);
    return EC_OK;
}


// 2 U node ids (a solid k-mer and its twin) must leave bit 31 (CYC) free
int check_node_ids(unsigned int U) {
    if (2ull * U >= (unsigned long long)CYC) {
        set_error("too many solid k-mers (%u) for 31-bit node ids", U);
        return EC_ERR_CAPACITY;
    }
    return EC_OK;
}

// the prescan's first byte outside {A,C,G,T,N} (Scalars::bad, ~0 = none) as EC_ERR_ALPHABET
int check_alphabet(const uint8_t *d_reads, unsigned long long bad) {
    if (bad == ~0ull) return EC_OK;
    uint8_t byte = 0;
    hipMemcpy(&byte, d_reads + bad, 1, hipMemcpyDeviceToHost);
    set_error("byte %llu (0x%02x) outside {A,C,G,T,N}", bad, byte);
    return EC_ERR_ALPHABET;
}
}  // namespace
