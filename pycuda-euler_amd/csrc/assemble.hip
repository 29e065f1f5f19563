// assemble.hip -- fused, device-resident restatement of the reference CPU assembler
//   build()        src/referenceassembler/referenceAssembler.py:25-42
//   all_contigs()  src/referenceassembler/referenceAssembler.py:79-111
// on MI355X (gfx950).  The reference walks an insertion-ordered Python dict sequentially;
// here every step is data-parallel and the dict order is recovered from per-string
// first-occurrence events (see DESIGN.md "Parallel formulation"):
//
//   prescan  thread/read : alphabet check, P, HyperLogLog(canonical)       -> table size
//   count    thread/read : rolling 2-bit fwd/rc codes, canonical key, open-addressing
//                          insert (64-bit CAS), count += 1|2, atomicMin first events
//   compact  thread/slot : count > limit -> dense solid arrays (wave ballot + 1 atomic/block)
//   links    thread/node : 8 neighbour probes -> out-degree + unique candidate, then the
//                          get_contig_forward extension rule -> succ / pred (oriented nodes)
//   rank     thread/node : Wyllie pointer jumping (head, rank, prefix-min of first events,
//                          cycle min-id + distance)
//   starts   thread/node : component start = oriented k-mer with the smallest first event
//                          (= first dict entry of its unitig); sort starts -> contig order
//   emit     thread/node : closed-form position of every node in its contig walk
//   gfa      thread/contig: heads/tails lookups -> G
#include "common.h"
#include "count_global.h"
#include "graph.h"

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <cmath>
#include <climits>
#include <cstring>
#include <cstddef>
#include <functional>
#include <type_traits>
#include <vector>

#include "count_part.h"
#include "count_v2.h"
#include "count_sk2.h"
#include "shard.h"
#include "compact.h"
#include "count_wide.h"
#include "hostin.h"
#include "join_w.h"
#include "extended.h"
#include "rank_tile.h"
#include "junction.h"
#include "join_local.h"
#include "clip.h"
#include "pop.h"
#include "spectrum.h"
#include "dense_filter.h"

#include <atomic>
#include <chrono>
#include <dlfcn.h>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <thread>

#include "session.h"
#include "count_phase.h"

namespace ec {

// all_contigs(d, k) from a caller's dict (referenceAssembler.py:79-111): entry i = (string,
// count) in dict order becomes an exchange record of its canonical key whose first event of
// the entry's orientation is i; a twin entry adds count 0 (build stores both strands with the
// same count).  bad gets the smallest entry index holding a byte outside ACGT.
template <typename Ops>
__global__ void __launch_bounds__(256) k_kmers_to_agg(const char *chars, const unsigned int *counts, uint64_t n, int k,
                                                      typename RecOf<typename Ops::K>::T *out, unsigned long long *bad) {
    using K = typename Ops::K;
    const K mask = Ops::mask(k);
    for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < n; t += (uint64_t)gridDim.x * blockDim.x) {
        const char *x = chars + t * (uint64_t)k;
        K code{};
        bool ok = true;
        for (int i = 0; i < k; i++) {
            const uint32_t b = base_code((unsigned char)x[i]);
            ok &= b < 4;
            code = Ops::push(code, b & 3u, mask);
        }
        if (!ok) atomicMin(bad, (unsigned long long)t);
        const K tw = Ops::twin(code, k);
        out[t] = RecOf<K>::make(code < tw ? code : tw, code <= tw ? counts[t] : 0u,
                                code <= tw ? (unsigned long long)t : ~0ull, tw <= code ? (unsigned long long)t : ~0ull);
    }
}
}  // namespace ec

namespace {

// the emission's three node maps set to NONE and its flag word cleared in one launch (four fills
// were four); n = nodes a map
__global__ void __launch_bounds__(256) k_emit_init(unsigned int *a, unsigned int *b, unsigned int *c, uint64_t n,
                                                   unsigned int *flag) {
    const uint64_t t0 = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x, st = (uint64_t)gridDim.x * blockDim.x;
    if (t0 == 0) *flag = 0;
    // (hipMalloc'd buffers: 16-byte aligned; the tail by single words)
    const uint64_t n4 = n / 4;
    const uint4 v = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
    uint4 *a4 = reinterpret_cast<uint4 *>(a), *b4 = reinterpret_cast<uint4 *>(b), *c4 = reinterpret_cast<uint4 *>(c);
    for (uint64_t i = t0; i < n4; i += st) {
        a4[i] = v;
        b4[i] = v;
        c4[i] = v;
    }
    for (uint64_t i = 4 * n4 + t0; i < n; i += st) a[i] = b[i] = c[i] = 0xFFFFFFFFu;
}

// elapsed times of the stage / kernel events recorded during this call (EC_FLAG_TIMING)
void collect_timing(ec_session *s) {
    if (!s->timing) return;
    hipStreamSynchronize(s->stream);
    for (int i = 0; i < EC_NSTAGES; i++) {
        float ms = 0;
        if (s->stage_timing && s->sused[i]) hipEventElapsedTime(&ms, s->ev[2 * i], s->ev[2 * i + 1]);
        s->stats.stage_ms[i] = ms;
    }
    for (int i = 0; i < EC_NKERNELS; i++) {
        float ms = 0;
        if (s->kused[i]) hipEventElapsedTime(&ms, s->kev[2 * i], s->kev[2 * i + 1]);
        s->stats.kernel_ms[i] = ms;
    }
}

// per-call setup shared by every entry point: argument checks, stats reset, timing events,
// zeroed device scalars
int begin_call(ec_session *s, int k, unsigned flags) {
    s->xalpha = false;  // (set by the extended-alphabet path, extended.h)
    // (the call rewrites the buffers a loaded / placed graph lives in, the dense arrays, and the
    // index and results ec_clip_tips reads; bucket marks of an earlier call never plan its tiles)
    drop_device_state(s, "the session's last call failed");
    refresh_knobs();
    s->have = false;
    s->stats_ok = false;
    if (k < 1 || k > EC_MAX_K) {
        set_error("k=%d outside [1,%d]", k, EC_MAX_K);
        return EC_ERR_ARG;
    }
    EC_HIP(hipSetDevice(s->device));
    // (an earlier call that failed may have left a results copy in flight on the output stream)
    if (s->ostream) EC_HIP(hipStreamSynchronize(s->ostream));
    memset(&s->stats, 0, sizeof(s->stats));
    s->k = k;
    s->want_dict = (flags & EC_FLAG_WANT_DICT) != 0;
    s->flags = flags;
    s->shard_base = 0;
    const bool timing = (flags & (EC_FLAG_TIMING | EC_FLAG_KERNEL_TIMING)) != 0;
    s->stage_timing = (flags & EC_FLAG_TIMING) != 0;
    if (timing && !s->events) {
        for (auto &e : s->ev) EC_HIP(hipEventCreate(&e));
        for (auto &e : s->kev) EC_HIP(hipEventCreate(&e));
        s->events = true;
    }
    s->timing = timing;
    for (auto &u : s->kused) u = false;
    for (auto &u : s->sused) u = false;
    EC_CHECK(s->scal.ensure(sizeof(Scalars)));
    s->jlspec.queued = false;
    s->graph_follows = false;
    k_scal_reset<<<1, 64, 0, s->stream>>>(s->scal.as<Scalars>());
    return EC_OK;
}

// palindrome flags of the canonical keys (k_upal).  Odd k over A/C/G/T has no palindromic
// k-mer (the middle base would be its own complement): the flags are a fill, not a pass over the
// keys (config 5: 0.64 ms of reading 3.2 GB of keys for nothing)
template <typename Ops>
inline int launch_upal(hipStream_t st, const typename Ops::K *dkey, unsigned int U, int k, uint8_t *upal,
                       unsigned int *npal) {
    if (!U) return EC_OK;
    if ((k & 1) && (std::is_same<Ops, Ops64>::value || std::is_same<Ops, OpsW>::value)) {
        EC_HIP(hipMemsetAsync(upal, 0, U, st));
        return EC_OK;
    }
    k_upal<Ops><<<grid_for(U, 256), 256, 0, st>>>(dkey, U, k, upal, npal);
    return EC_OK;
}

// Links by the (k-1)-mer half-edge join (join_w.h), 128-bit (OpsW) or 64-bit (Ops64) keys.
// gate: a device flag set when a level region or a join table overflowed; the caller then
// launches k_neighbors / k_succ gated on it (they return at once unless it is set).
template <typename Ops> struct JoinT;
template <> struct JoinT<OpsW> {
    using R = RecJ;
    using S = StoreJ;
    static void emit_l1(const K128 *d, unsigned U, int k, const uint8_t *up, int lb, uint64_t fc, unsigned long long *gc,
                        R *o, unsigned *ov, hipStream_t st) {
        k_half_emit_l1<K128, R><<<grid_for(U, 1024, 2048), 1024, 0, st>>>(d, U, k, up, lb, fc, gc, o, ov);
    }
    template <bool ODD>
    static void join(unsigned nb, const R *r, const unsigned long long *bb, const unsigned long long *be,
                     const uint8_t *up, unsigned *succ, unsigned *ov, hipStream_t st) {
        k_half_join<2048, 512, ODD><<<nb, 512, 0, st>>>(r, bb, be, up, succ, ov);
    }
};
struct JoinTM {  // 128-bit keys on minimizer-bucketed ids: junctions bucketed by their minimizer
    using R = RecJM;
    using S = StoreJM;
    static void emit_l1(const K128 *d, unsigned U, int k, const uint8_t *up, int lb, uint64_t fc, unsigned long long *gc,
                        R *o, unsigned *ov, hipStream_t st) {
        k_half_emit_l1<K128, R><<<grid_for(U, 1024, 2048), 1024, 0, st>>>(d, U, k, up, lb, fc, gc, o, ov);
    }
    template <bool ODD>
    static void join(unsigned nb, const R *r, const unsigned long long *bb, const unsigned long long *be,
                     const uint8_t *up, unsigned *succ, unsigned *ov, hipStream_t st) {
        k_half_join<2048, 512, ODD, RecJM><<<nb, 512, 0, st>>>(r, bb, be, up, succ, ov);
    }
};
template <> struct JoinT<Ops64> {
    using R = RecJ64;
    using S = StoreJ64;
    static void emit_l1(const unsigned long long *d, unsigned U, int k, const uint8_t *up, int lb, uint64_t fc,
                        unsigned long long *gc, R *o, unsigned *ov, hipStream_t st) {
        k_half_emit_l1<unsigned long long, R><<<grid_for(U, 1024, 2048), 1024, 0, st>>>(d, U, k, up, lb, fc, gc, o, ov);
    }
    template <bool ODD>
    static void join(unsigned nb, const R *r, const unsigned long long *bb, const unsigned long long *be,
                     const uint8_t *up, unsigned *succ, unsigned *ov, hipStream_t st) {
        k_half_join64<2048, 512, ODD><<<nb, 512, 0, st>>>(r, bb, be, up, succ, ov);
    }
};

template <typename Ops, typename J = JoinT<Ops>>
int links_join(ec_session *s, int k, unsigned int U, bool &ok, const unsigned int *&gate) {
    using R = typename J::R;
    using S = typename J::S;
    ok = false;
    hipStream_t st = s->stream;
    const unsigned B = 256;
    Scalars *dsc = s->scal.as<Scalars>();
    const uint64_t N = 2ull * U;
    // final buckets of <= 900 (k-1)-mer groups (~U of them) in 2048-slot tables; levels of <= 256
    int bt = 1;
    while ((double)U / (double)(1ull << bt) > 900.0) bt++;
    std::vector<int> lv;
    for (int rem = bt; rem > 0; rem -= std::min(8, rem)) lv.push_back(std::min(8, rem));
    uint64_t needA = 0, needB = 0, nbmax = 1;
    std::vector<uint64_t> fc(lv.size());
    for (size_t l = 0, cb = 0; l < lv.size(); l++) {
        cb += lv[l];
        const uint64_t nb = 1ull << cb, mean = N / nb;
        fc[l] = kn().join_cap > 0 ? (uint64_t)kn().join_cap : mean + mean * 3 / 10 + 1024;
        (l & 1 ? needA : needB) = std::max(l & 1 ? needA : needB, nb * fc[l]);
        nbmax = std::max(nbmax, nb);
    }
    EC_CHECK(s->recs.ensure(needA * sizeof(R)));
    EC_CHECK(s->recs2.ensure(needB * sizeof(R)));
    EC_CHECK(s->bb2.ensure(2 * nbmax * 8));
    EC_CHECK(s->gcur.ensure(nbmax * 8));
    EC_CHECK(s->tmp.ensure(16));
    unsigned int *flags = s->tmp.as<unsigned int>();  // [1]: a level region or a join table overflowed
    unsigned long long *ibeg = s->bb2.as<unsigned long long>(), *iend = ibeg + nbmax;
    EC_HIP(hipMemsetAsync(flags, 0, 8, st));
    const typename Ops::K *dkey = s->dkey.as<typename Ops::K>();
    EC_CHECK(launch_upal<Ops>(st, dkey, U, k, s->upal.as<uint8_t>(), &dsc->npal));
    R *src = s->recs.as<R>(), *dst = s->recs2.as<R>();
    // level 0 fused with the emit (k_half_emit_l1), its regions in dst
    const uint64_t nb0 = 1ull << lv[0];
    k_cursor_init<<<grid_for(nb0, B, 8192), B, 0, st>>>(s->gcur.as<unsigned long long>(), nb0, fc[0]);
    J::emit_l1(dkey, U, k, s->upal.as<uint8_t>(), lv[0], fc[0], s->gcur.as<unsigned long long>(), dst, &flags[1], st);
    k_level3_ends<<<grid_for(nb0, B, 8192), B, 0, st>>>(s->gcur.as<unsigned long long>(), nb0, fc[0], ibeg, iend);
    std::swap(src, dst);
    int cb = lv[0];
    for (size_t l = 1; l < lv.size(); l++) {
        const uint64_t nc = 1ull << cb, nb = 1ull << (cb + lv[l]);
        k_cursor_init<<<grid_for(nb, B, 8192), B, 0, st>>>(s->gcur.as<unsigned long long>(), nb, fc[l]);
        const unsigned rs = (unsigned)std::max<uint64_t>(1, 1024 / nc);
        k_refine<R, S, S><<<dim3((unsigned)nc, rs), BUCKET_THREADS, 0, st>>>(
            S{src}, S{dst}, nullptr, s->gcur.as<unsigned long long>(), cb, cb + lv[l], fc[l], &flags[1], ibeg, iend);
        k_level3_ends<<<grid_for(nb, B, 8192), B, 0, st>>>(s->gcur.as<unsigned long long>(), nb, fc[l], ibeg, iend);
        std::swap(src, dst);
        cb += lv[l];
    }
    EC_HIP(hipMemsetAsync(s->succ.p, 0xFF, N * 4, st));
    if (k & 1)
        J::template join<true>((unsigned)(1ull << cb), src, ibeg, iend, s->upal.as<uint8_t>(), s->succ.as<unsigned int>(),
                               &flags[1], st);
    else
        J::template join<false>((unsigned)(1ull << cb), src, ibeg, iend, s->upal.as<uint8_t>(),
                                s->succ.as<unsigned int>(), &flags[1], st);
    // no host round trip: the caller's probe kernels run gated on flags[1] (a level region or a
    // join table that overflowed) and then rewrite every successor
    gate = &flags[1];
    ok = true;
    return EC_OK;
}

// Links joined inside the count's minimizer tables (join_local.h): keys on tables of ids grouped
// by table -- the super-k-mer count's minimizer tables (64-bit), the wide minimizer count's
// (128-bit).  ok = false: not such an index (the caller takes links_join).
template <typename Index>
inline int jl_bits(const Index &) { return -1; }
template <>
inline int jl_bits<SolidIndex>(const SolidIndex &x) { return x.sub && x.sk && !x.npb && !x.bijk ? x.bbits : -1; }
template <>
inline int jl_bits<SolidIndexW>(const SolidIndexW &x) { return x.sub && x.mb ? x.bbits : -1; }

// the local join's per-key table words, table id ranges, foreign counts / offsets and flags for
// u keys in ntab tables (links_local, and links_prologue on the previous call's shape)
int jl_ensure(ec_session *s, unsigned int u, unsigned int ntab) {
    EC_CHECK(s->jl_kof.ensure((size_t)u * 4));
    EC_CHECK(s->jl_rs.ensure((size_t)ntab * 4));
    EC_CHECK(s->jl_re.ensure((size_t)ntab * 4));
    EC_CHECK(s->jl_cnt.ensure(((size_t)ntab + 1) * 4));
    EC_CHECK(s->jl_off.ensure(((size_t)ntab + 1) * 4));
    EC_CHECK(s->jl_flag.ensure((size_t)(JL_NCTR + 1) * JL_CSTRIDE * 4));
    return EC_OK;
}

// The graph phase's first kernels queued by phase_count_sk2 (count_phase.h) behind its bucket
// kernel while the host waits for the solid count (a ~26 us hole on the headline: wake-up, plan,
// allocations' checks, first launch): links_local's k_jl_init and k_jl_scan on the previous call's
// shape, the scan reading U from the device.  count_stands: the count's side of the gate -- its
// first pass, the speculative refine stood (a stream of like batches), no filter, no statistics;
// the rest is here: a call that goes on to phase_graph, odd k, the previous call's tables.
// links_local takes the prologue over if the count stood (no overflow, no second refine) and U
// fits, and runs its own otherwise.  It writes nothing the count's redo paths read: the foreign
// records go to jl_frec, not to s->recs (the second refine's input).
// waited: the prologue ran and the host has waited for the scalars' read-back (hsc, queued by
// the caller before the call) on an event recorded before it; false: nothing queued, no wait
int links_prologue(ec_session *s, int k, int bbits, bool count_stands, const Scalars &hsc, bool &waited) {
    hipStream_t st = s->stream;
    Scalars *dsc = s->scal.as<Scalars>();
    const auto jp = s->jlspec;
    s->jlspec.queued = false;
    waited = false;
    if (!(count_stands && jp.valid && s->graph_follows && !s->no_index && (k & 1) && jp.k == k && jp.bits == bbits &&
          kn().jl_bits_delta == 0 && kn().jl_fcap <= 0 && kn().join_links != 0 && kn().join_local != 0))
        return EC_OK;
    const unsigned int ntab = 1u << jp.bits;
    EC_CHECK(jl_ensure(s, jp.ucap, ntab));
    EC_CHECK(s->jl_frec.ensure((size_t)jp.fcap * sizeof(RecJ64)));
    EC_CHECK(s->upal.ensure(jp.ucap));
    EC_CHECK(s->succ.ensure((size_t)jp.ucap * 8));
    if (!s->rd_ev) EC_HIP(hipEventCreateWithFlags(&s->rd_ev, hipEventDisableTiming));
    EC_HIP(hipEventRecord(s->rd_ev, st));
    unsigned int *flags = s->jl_flag.as<unsigned int>();
    k_jl_init<<<grid_for(2ull * jp.ucap, 256, 4096), 256, 0, st>>>(
        flags, (JL_NCTR + 1) * JL_CSTRIDE, s->jl_rs.as<unsigned int>(), s->jl_cnt.as<unsigned int>(), ntab,
        s->succ.as<unsigned int>(), 2ull * jp.ucap, s->upal.as<uint8_t>(), jp.ucap);
    k_jl_scan<unsigned long long><<<grid_for(jp.ucap, 256, 8192), 256, 0, st>>>(
        s->dkey.as<unsigned long long>(), jp.ucap, k, jp.bits, s->upal.as<uint8_t>(), s->jl_kof.as<unsigned int>(),
        s->jl_frec.as<RecJ64>(), flags + JL_CSTRIDE, jp.fcap, s->jl_cnt.as<unsigned int>(),
        s->jl_rs.as<unsigned int>(), s->jl_re.as<unsigned int>(), &flags[1], &dsc->nsolid, &flags[2]);
    EC_CHECK(host_wait(s, s->rd_ev));
    waited = true;
    // (the scan held U to ucap: a larger count, like an overflow, leaves the prologue unused;
    // phase_graph counts a prologue links_local did not take over as redone)
    s->jlspec.queued = true;
    if (hsc.skew || hsc.overflow || hsc.nsolid > jp.ucap) {
        s->jlspec.queued = false;
        s->spec_cnt[1]++;
    }
    return EC_OK;
}

template <typename Ops, typename Index>
int links_local(ec_session *s, int k, unsigned int U, const Index &sidx, bool &ok, const unsigned int *&gate) {
    using K = typename Ops::K;
    using R = typename JLRec<K>::R;
    ok = false;
    int bits = jl_bits(sidx);
    if (bits < 1 || bits > 22 || k < SK_M + 2) return EC_OK;
    // (tests: tables finer or coarser than the count's -- ids not grouped by table, the gate opens)
    if (kn().jl_bits_delta) bits = std::max(1, std::min(22, bits + kn().jl_bits_delta));
    const unsigned int ntab = 1u << bits;
    // a table's junction groups ~ its keys (plus the foreign records sent to it): tables of mean
    // <= ~700 keys in 2048 slots, <= ~1500 in 4096 (an overflowing one opens the gate)
    const double mean = (double)U / ntab;
    const int slots = mean <= 700.0 ? 2048 : mean <= 1500.0 ? 4096 : 0;
    if (!slots) return EC_OK;
    hipStream_t st = s->stream;
    const unsigned B = 256;
    Scalars *dsc = s->scal.as<Scalars>();
    const uint64_t N = 2ull * U;
    // foreign records: ~2 / (w + 1) of the 2U (7 % at k = 31, 3 % at k = 51); room for a third
    auto fcap_of = [](unsigned int u) { return (u / 3 / JL_NCTR + 64) * JL_NCTR; };
    unsigned int fcap = kn().jl_fcap > 0 ? ((unsigned int)kn().jl_fcap / JL_NCTR + 1) * JL_NCTR : fcap_of(U);
    // phase_count_sk2's prologue (k_jl_init, k_jl_scan on the previous call's shape) stands when it
    // assumed this call's tables and its capacities hold U: its foreign records, in regions of its
    // own (larger) capacity, are in jl_frec
    const auto jp = s->jlspec;
    const bool pro = jp.queued && std::is_same<K, unsigned long long>::value && jp.bits == bits && jp.k == k &&
                     U <= jp.ucap && jp.fcap >= fcap && kn().jl_fcap <= 0;
    s->jlspec = ec_session::JlSpec{};
    if (jp.queued && !pro) s->spec_cnt[1]++;  // (redone below)
    if (pro) fcap = jp.fcap;
    EC_CHECK(jl_ensure(s, U, ntab));
    if (!pro) EC_CHECK(s->recs.ensure((size_t)fcap * sizeof(R)));
    EC_CHECK(s->recs2.ensure((size_t)fcap * sizeof(R)));
    // [1]: the gate; [2]: the prologue's U past its capacity; [JL_CSTRIDE (r + 1)]: foreign records of region r
    unsigned int *flags = s->jl_flag.as<unsigned int>(), *fctr = flags + JL_CSTRIDE;
    unsigned int *cnt = s->jl_cnt.as<unsigned int>(), *off = s->jl_off.as<unsigned int>();
    const K *dkey = s->dkey.as<K>();
    uint8_t *upal = s->upal.as<uint8_t>();
    const R *frec = pro ? s->jl_frec.as<R>() : s->recs.as<R>();
    if (pro) {
        s->spec_cnt[0]++;
    } else {
    // (odd k: no palindromic k-mer, the flags a fill in the same launch; even k: k_upal)
    k_jl_init<<<grid_for(N, B, 4096), B, 0, st>>>(flags, (JL_NCTR + 1) * JL_CSTRIDE, s->jl_rs.as<unsigned int>(), cnt,
                                                 ntab, s->succ.as<unsigned int>(), N, (k & 1) ? upal : nullptr, U);
    if (!(k & 1)) EC_CHECK(launch_upal<Ops>(st, dkey, U, k, upal, &dsc->npal));
    k_jl_scan<K><<<grid_for(U, B, 8192), B, 0, st>>>(dkey, U, k, bits, upal, s->jl_kof.as<unsigned int>(), s->recs.as<R>(),
                                                     fctr, fcap, cnt, s->jl_rs.as<unsigned int>(),
                                                     s->jl_re.as<unsigned int>(), &flags[1]);
    }
    k_jl_edges<<<grid_for(U / 64 + 2, B, 4096), B, 0, st>>>(s->jl_kof.as<unsigned int>(), U, s->jl_rs.as<unsigned int>(),
                                                           s->jl_re.as<unsigned int>(), &flags[1]);
    EC_CHECK(scan_excl_u32(s, cnt, off, (size_t)ntab + 1));
    k_jl_scatter<R><<<grid_for(fcap, B, 4096), B, 0, st>>>(frec, fctr, fcap, off, cnt, s->recs2.as<R>());
    // (4096 slots: 96 KB of 128-bit slots, one workgroup a CU -- 512 threads to hide the probes)
#define EC_JL_JOIN(SL, ODD)                                                                                        \
    k_jl_join<K, SL, SL / 8, ODD><<<ntab, SL / 8, 0, st>>>(dkey, s->jl_kof.as<unsigned int>(), s->jl_rs.as<unsigned int>(), \
                                                     s->jl_re.as<unsigned int>(), k, upal, s->recs2.as<R>(), off,     \
                                                     s->succ.as<unsigned int>(), &flags[1])
    if (slots == 2048) {
        if (k & 1) EC_JL_JOIN(2048, true);
        else EC_JL_JOIN(2048, false);
    } else {
        if (k & 1) EC_JL_JOIN(4096, true);
        else EC_JL_JOIN(4096, false);
    }
#undef EC_JL_JOIN
    EC_HIP(hipGetLastError());
    gate = &flags[1];
    ok = true;
    // what the next call's prologue may assume: these tables, and room for a sixteenth more keys
    // (batches of a stream differ a little; its init and scan pay for the room they do not use)
    if (std::is_same<K, unsigned long long>::value && kn().no_spec == 0) {
        s->jlspec.valid = true;
        s->jlspec.bits = bits;
        s->jlspec.k = k;
        s->jlspec.ucap = (unsigned int)std::min<uint64_t>((uint64_t)U + U / 16 + 64, (uint64_t)CYC / 2 - 1);
        s->jlspec.fcap = fcap_of(s->jlspec.ucap);
    }
    return EC_OK;
}

// rank_tile.h (2): the super list srec (M chains, SIDX[head] = index) linked and ranked by the
// weighted ruling set; per chain its path key / rank (rt_pks / rt_rks), paths' and cycles'
// length / min first event at their key nodes (PL / PM)
int rank_supers(ec_session *s, unsigned int M, unsigned int N, unsigned int &nr, int &rounds,
                bool pre_init = false, const unsigned int *sidx = nullptr) {
    hipStream_t st = s->stream;
    const unsigned B = 256;
    Scalars *dsc = s->scal.as<Scalars>();
    Scalars hsc{};
    SuperRec *srec = s->rt_srec.as<SuperRec>();
    // (sidx: head node -> super index; the look-back compaction's LH serves, being that at heads)
    const unsigned int *SIDX = sidx ? sidx : s->rt_sidx.as<unsigned int>();
    const size_t cap = std::max<size_t>(M, 1);
    EC_CHECK(s->rt_snrec.ensure(cap * sizeof(SNodeRec)));
    EC_CHECK(s->rt_hasp.ensure(cap));
    EC_CHECK(s->rt_pks.ensure(cap * 4));
    EC_CHECK(s->rt_rks.ensure(cap * 4));
    EC_CHECK(s->rid.ensure(cap * 8));
    EC_CHECK(s->rlist.ensure(cap * 4));
    EC_CHECK(s->nextR.ensure(cap * 4));
    EC_CHECK(s->st0.ensure(cap * sizeof(RJump)));
    EC_CHECK(s->st1.ensure(cap * sizeof(RJump)));
    EC_CHECK(s->rbc.ensure(((cap + RULER_CHUNK - 1) / RULER_CHUNK) * 8 + 8));
    SNodeRec *snrec = s->rt_snrec.as<SNodeRec>();
    if (!pre_init) EC_HIP(hipMemsetAsync(s->rt_hasp.p, 0, M, st));  // (pre_init: k_tile_compact did these)
    k_super_link<<<grid_for(M, B), B, 0, st>>>(srec, M, SIDX, snrec, s->rt_hasp.as<uint8_t>());
    if (!pre_init) {
        EC_HIP(hipMemsetAsync(s->rid.p, 0xFF, (size_t)M * 8, st));
        EC_HIP(hipMemsetAsync(&dsc->nr, 0, 4, st));
        EC_HIP(hipMemsetAsync(&dsc->nvisited, 0, 8, st));
    }
    const unsigned int masks[4] = {15u, 3u, 1u, 0u};
    unsigned int r0 = 0;
    const unsigned int nblk = (M + RULER_CHUNK - 1) / RULER_CHUNK;
    for (int it = 0; it < 4; it++) {
        k_srulers_count<<<nblk, B, 0, st>>>(s->rt_hasp.as<uint8_t>(), M, masks[it], it == 0, s->rid.as<uint2>(),
                                            s->rbc.as<unsigned int>());
        EC_CHECK(scan_incl_u32(s, s->rbc.as<unsigned int>(), s->rbc.as<unsigned int>() + nblk, nblk));
        k_srulers<<<nblk, B, 0, st>>>(s->rt_hasp.as<uint8_t>(), M, masks[it], it == 0, s->rbc.as<unsigned int>() + nblk,
                                      &dsc->nr, s->rid.as<uint2>(), s->rlist.as<unsigned int>());
        k_rulers_total<<<1, 1, 0, st>>>(s->rbc.as<unsigned int>() + nblk, nblk, &dsc->nr);
        k_walk_s<<<2048, B, 0, st>>>(snrec, s->rlist.as<unsigned int>(), r0, &dsc->nr, masks[it], s->rid.as<uint2>(),
                                     s->nextR.as<unsigned int>(), s->st0.as<RJump>(), &dsc->nvisited, srec);
        EC_CHECK(d2h(s, &hsc, dsc, sizeof(Scalars), st));
        EC_CHECK(host_sync(s, st));
        r0 = hsc.nr;
        if (hsc.nvisited >= M) break;
    }
    nr = hsc.nr;
    if (hsc.nvisited != M) {
        set_error("ruling set covered %llu of %u chains", (unsigned long long)hsc.nvisited, M);
        return EC_ERR_STATE;
    }
    k_rjump_init<<<grid_for(nr, B), B, 0, st>>>(s->nextR.as<unsigned int>(), nr, s->st0.as<RJump>());
    rounds = 1;
    while ((1ull << (rounds - 1)) < (unsigned long long)nr) rounds++;
    rounds = std::min(rounds + 1, 63);
    RJump *bufs[2] = {s->st0.as<RJump>(), s->st1.as<RJump>()};
    // (the rounds only raise their flags: clear what an unconverged queued ranking left)
    EC_HIP(hipMemsetAsync(dsc->active, 0, sizeof(dsc->active), st));
    for (int r = 0; r < rounds; r++)
        k_rjump<<<grid_for(nr, B), B, 0, st>>>(bufs[r & 1], bufs[(r + 1) & 1], nr, N, r ? &dsc->active[r - 1] : nullptr,
                                              &dsc->active[r], &dsc->final_sel, (unsigned)((r + 1) & 1));
    k_finalize_s<<<grid_for(M, B), B, 0, st>>>(snrec, srec, s->rid.as<uint2>(), s->rlist.as<unsigned int>(), bufs[0],
                                              bufs[1], &dsc->final_sel, &dsc->active[rounds - 1], M,
                                              s->rt_pks.as<unsigned int>(), s->rt_rks.as<unsigned int>(),
                                              s->PL.as<unsigned int>(), s->PM.as<unsigned long long>());
    k_cycle_len_s<<<grid_for(nr, B), B, 0, st>>>(s->nextR.as<unsigned int>(), s->rlist.as<unsigned int>(), srec, bufs[0],
                                                bufs[1], &dsc->final_sel, &dsc->active[rounds - 1], nr,
                                                s->PL.as<unsigned int>(), s->PM.as<unsigned long long>());
    return EC_OK;
}

// rank_supers without host read-backs: the chain count M and the ruler count stay on the device
// (dM, Scalars::nr), grids are sized by the node count N >= M and read the counts in-kernel,
// one ruler pass only (mask 15 plus every head), Wyllie rounds for N rulers (rounds past
// convergence exit at once).  The whole ranking is queued while the device still runs the links:
// after a read-back the host issued these ~25 launches slower than the device ran them
// (~0.25 ms from the walk to finalize on the headline).  Chains no ruler reached (a cycle of
// chains without a sampled one) are caught by the caller's next scalar read (nvisited < M),
// which redoes the ranking with rank_supers.  Needs k_tile_compact's initialisation (pre_init).
int rank_supers_async(ec_session *s, unsigned int N, const unsigned long long *dM, int &rounds,
                      unsigned int mcap = 0, const unsigned int *sidx = nullptr) {
    // mcap: a bound of the chain count known on the host (the partitioned finish's gathered
    // list) -- grids and Wyllie rounds sized by it instead of the node count N, which stays the
    // cycle bound of the jumps (j.s < N)
    const unsigned int G = mcap ? mcap : N;
    hipStream_t st = s->stream;
    const unsigned B = 256;
    Scalars *dsc = s->scal.as<Scalars>();
    SuperRec *srec = s->rt_srec.as<SuperRec>();
    // (buffers sized by N, not by the chain count, when the count is only on the device: a count a
    // little above the last call's would reallocate them; with mcap, by it with part_rank's spare
    // -- the gathered list of the partitioned finish is far below its node count)
    const size_t cap = mcap ? (size_t)mcap + 4096 : std::max<size_t>(N, 1);
    const unsigned int spare = mcap ? 16u : 0u;
    EC_CHECK(s->rt_snrec.ensure(cap * sizeof(SNodeRec), spare));
    EC_CHECK(s->rt_pks.ensure(cap * 4, spare));
    EC_CHECK(s->rt_rks.ensure(cap * 4, spare));
    EC_CHECK(s->rlist.ensure(cap * 4, spare));
    EC_CHECK(s->nextR.ensure(cap * 4, spare));
    EC_CHECK(s->rbc.ensure(((cap + RULER_CHUNK - 1) / RULER_CHUNK) * 8 + 8, spare));
    SNodeRec *snrec = s->rt_snrec.as<SNodeRec>();
    const unsigned int *dnr = &dsc->nr;
    const unsigned int gs = std::min(grid_for(G, B), 4096u);  // grid-stride grids over <= G items
    k_super_link<<<gs, B, 0, st>>>(srec, 0, sidx ? sidx : s->rt_sidx.as<unsigned int>(), snrec,
                                   s->rt_hasp.as<uint8_t>(), dM);
    const unsigned int smask = 15u;
    const unsigned int nblk = (G + RULER_CHUNK - 1) / RULER_CHUNK;
    k_srulers_count<<<nblk, B, 0, st>>>(s->rt_hasp.as<uint8_t>(), 0, smask, 1, s->rid.as<uint2>(),
                                        s->rbc.as<unsigned int>(), dM);
    EC_CHECK(scan_incl_u32(s, s->rbc.as<unsigned int>(), s->rbc.as<unsigned int>() + nblk, nblk));
    k_srulers<<<nblk, B, 0, st>>>(s->rt_hasp.as<uint8_t>(), 0, smask, 1, s->rbc.as<unsigned int>() + nblk, &dsc->nr,
                                  s->rid.as<uint2>(), s->rlist.as<unsigned int>(), dM);
    k_rulers_total<<<1, 1, 0, st>>>(s->rbc.as<unsigned int>() + nblk, nblk, &dsc->nr);
    k_walk_s<<<2048, B, 0, st>>>(snrec, s->rlist.as<unsigned int>(), 0, &dsc->nr, smask, s->rid.as<uint2>(),
                                 s->nextR.as<unsigned int>(), s->st0.as<RJump>(), &dsc->nvisited, srec);
    // rulers <= chains <= N: rounds for N (a round after convergence returns at its first load)
    const unsigned int gr = std::min(grid_for(G / 8u + 1, B), 2048u);
    k_rjump_init<<<gr, B, 0, st>>>(s->nextR.as<unsigned int>(), 0, s->st0.as<RJump>(), dnr);
    rounds = 1;
    while ((1ull << (rounds - 1)) < (unsigned long long)G) rounds++;
    rounds = std::min(rounds + 1, 63);
    if (s->spec_rounds > 0 && s->spec_rounds < rounds) rounds = s->spec_rounds;
    RJump *bufs[2] = {s->st0.as<RJump>(), s->st1.as<RJump>()};
    for (int r = 0; r < rounds; r++)
        k_rjump<<<gr, B, 0, st>>>(bufs[r & 1], bufs[(r + 1) & 1], 0, N, r ? &dsc->active[r - 1] : nullptr,
                                  &dsc->active[r], &dsc->final_sel, (unsigned)((r + 1) & 1), dnr);
    k_finalize_s<<<gs, B, 0, st>>>(snrec, srec, s->rid.as<uint2>(), s->rlist.as<unsigned int>(), bufs[0], bufs[1],
                                   &dsc->final_sel, &dsc->active[rounds - 1], 0, s->rt_pks.as<unsigned int>(),
                                   s->rt_rks.as<unsigned int>(), s->PL.as<unsigned int>(),
                                   s->PM.as<unsigned long long>(), dM);
    k_cycle_len_s<<<gr, B, 0, st>>>(s->nextR.as<unsigned int>(), s->rlist.as<unsigned int>(), srec, bufs[0], bufs[1],
                                    &dsc->final_sel, &dsc->active[rounds - 1], 0, s->PL.as<unsigned int>(),
                                    s->PM.as<unsigned long long>(), dnr);
    return EC_OK;
}

// contig characters -> 2-bit codes (A C G T = 0..3, pack4's mapping), 16 characters a thread,
// up to *total (the contigs' offsets' last entry) of them; the bytes past it are padding
__global__ void __launch_bounds__(256) k_pack_chars(const uint4 *chars, const unsigned long long *total, uint64_t cap16,
                                                    uint32_t *codes) {
    const uint64_t n16 = min<uint64_t>((*total + 15) / 16, cap16);
    for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < n16; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint4 v = chars[t];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        uint32_t out = 0;
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint32_t x = ((w[u] >> 1) ^ (w[u] >> 2)) & 0x03030303u;  // A C G T -> 0 1 2 3 per byte
            const uint32_t y = x | (x >> 6);
            out |= ((y | (y >> 12)) & 0xFFu) << (8 * u);
        }
        codes[t] = out;
    }
}

// the rounds a ranking used (the last round that still moved a pointer + 1), for the next
// call's speculation; 0 when the last round still moved one (not converged)
constexpr unsigned int OCOPY_MIN = 1u << 16;  // contigs past which results copy on the output stream
int rounds_used(const Scalars &h, int rounds) {
    if (rounds <= 0 || h.active[rounds - 1]) return 0;
    int used = 1;
    for (int r = 0; r < rounds; r++)
        if (h.active[r]) used = r + 2;
    return std::min(used, rounds);
}
void note_rounds(ec_session *s, const Scalars &h, int rounds) {
    const int used = rounds_used(h, rounds);
    s->spec_rounds = used ? used + 1 : 0;
}

// extended alphabet (extended.h): links without their twin link make their components'
// walks overlap; those components are cut out of the parallel ranking (their successors saved
// in x_succ) and their dict entries listed in (component, first event) order for k_x_emulate.
// nx = the entries listed (0: every link has its twin link, nothing to do)
int x_cut(ec_session *s, unsigned int U, unsigned int &nx) {
    hipStream_t st = s->stream;
    const unsigned B = 256;
    Scalars *dsc = s->scal.as<Scalars>();
    const unsigned int N = 2 * U;
    nx = 0;
    EC_HIP(hipMemsetAsync(&dsc->nasym, 0, 16, st));  // nasym, nxl, nxs, xbad
    k_x_asym<<<grid_for(N, B), B, 0, st>>>(s->upal.as<uint8_t>(), s->succ.as<unsigned int>(), N, &dsc->nasym);
    unsigned int nasym = 0;
    EC_CHECK(d2h(s, &nasym, &dsc->nasym, 4, st));
    EC_CHECK(host_sync(s, st));
    if (kn().verbose) fprintf(stderr, "extended: %u one-way links among %u nodes\n", nasym, N);
    if (!nasym) return EC_OK;
    EC_CHECK(s->x_par.ensure((size_t)U * 4));
    EC_CHECK(s->x_irr.ensure(U));
    EC_CHECK(s->x_in.ensure(U));
    EC_CHECK(s->x_succ.ensure((size_t)N * 4));
    EC_CHECK(s->x_lk.ensure((size_t)N * 8));
    EC_CHECK(s->x_lk2.ensure((size_t)N * 8));
    EC_CHECK(s->x_lv.ensure((size_t)N * 4));
    EC_CHECK(s->x_lv2.ensure((size_t)N * 4));
    // union-find over canonical ids (CAS hooks); par then holds the roots (the tree in x_lv2)
    unsigned int *par = s->x_par.as<unsigned int>(), *tree = s->x_lv2.as<unsigned int>();
    k_x_iota<<<grid_for(U, B), B, 0, st>>>(tree, U);
    k_x_uf_link<<<grid_for(N, B), B, 0, st>>>(s->upal.as<uint8_t>(), s->succ.as<unsigned int>(), N, tree);
    k_x_uf_flatten<<<grid_for(U, B), B, 0, st>>>(U, tree, par);
    EC_HIP(hipMemsetAsync(s->x_irr.p, 0, U, st));
    k_x_mark_irr<<<grid_for(N, B), B, 0, st>>>(s->upal.as<uint8_t>(), s->succ.as<unsigned int>(), N, par,
                                              s->x_irr.as<uint8_t>());
    k_x_cut<<<grid_for(N, B), B, 0, st>>>(s->upal.as<uint8_t>(), N, par, s->x_irr.as<uint8_t>(), s->x_in.as<uint8_t>(),
                                         s->succ.as<unsigned int>(), s->x_succ.as<unsigned int>(),
                                         s->dfc.as<unsigned long long>(), s->dft.as<unsigned long long>(),
                                         s->x_lk.as<unsigned long long>(), s->x_lv.as<unsigned int>(), &dsc->nxl);
    EC_CHECK(d2h(s, &nx, &dsc->nxl, 4, st));
    EC_CHECK(host_sync(s, st));
    if (kn().verbose) fprintf(stderr, "extended: %u one-way links, %u dict entries in their components\n", nasym, nx);
    // (component, first event) order: by event, then stably by component root
    EC_CHECK(sort_pairs(s, s->x_lk.as<unsigned long long>(), s->x_lk2.as<unsigned long long>(), s->x_lv.as<unsigned int>(),
                        s->x_lv2.as<unsigned int>(), nx));
    k_x_rekey<<<grid_for(nx, B), B, 0, st>>>(s->x_lv2.as<unsigned int>(), nx, par, s->x_lk.as<unsigned long long>());
    EC_CHECK(sort_pairs(s, s->x_lk.as<unsigned long long>(), s->x_lk2.as<unsigned long long>(),
                        s->x_lv2.as<unsigned int>(), s->x_lv.as<unsigned int>(), nx));
    return EC_OK;
}

// dense ids with minimizer locality (a bucket's ids contiguous, a bucket = whole minimizers:
// the super-k-mer count, the sharded load on minimizer buckets): most links stay inside a
// rank_tile.h tile.  Hash-bucketed ids (window records, 128-bit keys, extended alphabet) have
// none -- every link would leave its tile and the contraction only add work
template <typename Index>
inline bool ids_minimizer_local(const Index &) { return false; }
template <>
inline bool ids_minimizer_local<SolidIndex>(const SolidIndex &x) { return x.sk != 0; }
template <>
inline bool ids_minimizer_local<SolidIndexW>(const SolidIndexW &x) { return x.mb != 0; }

// the index of the set a one-GPU graph phase ran on, kept for ec_clip_tips' window lookups
inline void keep_index(ec_session *s, const SolidIndex &x) { s->cidx = x; }
inline void keep_index(ec_session *s, const SolidIndexW &x) { s->cidxw = x; }

// ---- the graph phase's stages, in the order phase_graph (below) runs them ------------------------
// links: palindrome flags and successors of the U solid k-mers' 2U oriented nodes -- the ranks'
// partitioned links copied (ext_succ), or joined inside the count's minimizer tables
// (join_local.h), joined globally (join_w.h), or probed (k_neighbors; after a join only where it
// overflowed) -- then the extended alphabet's cut (nx: dict entries of its components with one-way
// links), and for the node ranking pred with the first ruler pass's counts
template <typename Ops, typename Index>
int graph_links(ec_session *s, int k, unsigned int U, const Index &sidx, const unsigned int *ext_succ, bool tile_rank,
                unsigned int &nx) {
    hipStream_t st = s->stream;
    const unsigned B = 256;
    Scalars *dsc = s->scal.as<Scalars>();
    const unsigned int N = 2 * U;
    const size_t Nn = std::max<size_t>(N, 1);
    nx = 0;
    EC_CHECK(s->upal.ensure(std::max<size_t>(U, 1)));
    EC_CHECK(s->outdeg.ensure(std::max<size_t>(Nn, (Nn / 64 + 8) * 8)));  // (later: k_pred_rc's ruler bits)
    EC_CHECK(s->cand.ensure(Nn * 4));
    EC_CHECK(s->succ.ensure(Nn * 4));
    EC_CHECK(s->pred.ensure(Nn * 4));
    if (U && ext_succ) {  // partitioned links (ec_graph_finish): successors computed by the ranks
        EC_CHECK(launch_upal<Ops>(st, s->dkey.as<typename Ops::K>(), U, k, s->upal.as<uint8_t>(), &dsc->npal));
        EC_HIP(hipMemcpyAsync(s->succ.p, ext_succ, (size_t)N * 4, hipMemcpyDeviceToDevice, st));
    }
    // links by the half-edge join (join_w.h) instead of neighbour probes from ~2e6 keys on, for
    // every index (measured on the headline's minimizer index, round 4: links 0.34 ms joined
    // against 0.50 ms probed, EULERHIP_JOIN_LINKS=0)
    bool joined = false, local = false;
    const unsigned int *gate = nullptr;
    constexpr bool XT = std::is_same<Ops, OpsX>::value;  // extended alphabet (extended.h)
    if constexpr (!XT) {
        // inside the count's minimizer tables first (join_local.h), when the ids are grouped so
        if (U && !ext_succ && kn().join_links != 0 && kn().join_local != 0 &&
            (kn().join_local == 1 || kn().join_links == 1 || U >= (1u << 21))) {
            EC_CHECK(links_local<Ops>(s, k, U, sidx, joined, gate));
            local = joined;
        }
    }
    // (a prologue phase_count_sk2 queued and links_local did not take over: redone, or not needed;
    // without a local join this call, the next call has no shape to assume)
    if (s->jlspec.queued) s->spec_cnt[1]++;
    if (!local || s->jlspec.queued) s->jlspec = ec_session::JlSpec{};
    if constexpr (!XT) {
        if (!joined && U && !ext_succ && k >= 8 && kn().join_links != 0 && (kn().join_links == 1 || U >= (1u << 21)))
        {
            if constexpr (std::is_same<Index, SolidIndexW>::value) {
                // (opt-in: config 5's junction groups overflowed the join's fixed-capacity regions,
                // sized for uniform hashes, and the probe fallback took links 39 -> 81 ms)
                if (sidx.mb && kn().join_mb == 1) EC_CHECK((links_join<Ops, JoinTM>(s, k, U, joined, gate)));
                else EC_CHECK(links_join<Ops>(s, k, U, joined, gate));
            } else {
                EC_CHECK(links_join<Ops>(s, k, U, joined, gate));
            }
        }
    }
    if (U && !ext_succ) {  // (after a join: only if it overflowed, decided on the device)
        // gated: a small grid-stride grid, so the normal case (the gate closed) costs ~2 us a
        // launch instead of one exiting block per 256 nodes
        const unsigned gn = joined ? std::min(grid_for(N, B), 2048u) : grid_for(N, B);
        k_neighbors<Ops, Index><<<gn, B, 0, st>>>(sidx, s->dkey.as<typename Ops::K>(), U, k,
                                                 s->upal.as<uint8_t>(), s->outdeg.as<uint8_t>(),
                                                 s->cand.as<unsigned int>(), joined ? nullptr : &dsc->npal, gate);
        // (the node records only where k_succ writes them: tile ranking never reads them, and
        // after a join k_pred_rc writes them)
        NodeRec *nrec = nullptr;
        if (!(joined || tile_rank)) {
            EC_CHECK(s->nrec.ensure(Nn * sizeof(NodeRec)));
            nrec = s->nrec.as<NodeRec>();
        }
        k_succ<<<gn, B, 0, st>>>(s->upal.as<uint8_t>(), s->outdeg.as<uint8_t>(), s->cand.as<unsigned int>(), N,
                                s->succ.as<unsigned int>(), s->dfc.as<unsigned long long>(),
                                s->dft.as<unsigned long long>(), nrec, gate);
    }
    if constexpr (XT) {
        if (U) EC_CHECK(x_cut(s, U, nx));
    }
    if (U && !tile_rank) {
        // (with the first ruler pass's counts: rank_nodes skips k_rulers_count at it = 0, and the
        // node records when k_succ did not write them, or wrote successors x_cut has cut since)
        EC_CHECK(s->nrec.ensure(Nn * sizeof(NodeRec)));
        EC_CHECK(s->rbc.ensure(((Nn + RULER_CHUNK - 1) / RULER_CHUNK) * 8));
        k_pred_rc<<<(unsigned int)((N + RULER_CHUNK - 1) / RULER_CHUNK), B, 0, st>>>(
            s->upal.as<uint8_t>(), s->succ.as<unsigned int>(), N, 31u, s->pred.as<unsigned int>(),
            s->rbc.as<unsigned int>(), s->dfc.as<unsigned long long>(), s->dft.as<unsigned long long>(),
            (ext_succ || joined || nx) ? s->nrec.as<NodeRec>() : nullptr, s->outdeg.as<unsigned long long>());
    }
    return EC_OK;
}

// what a ranking leaves for the starts
struct Ranked {
    unsigned int nr = 0;  // rulers
    int rounds = 0;       // Wyllie rounds launched (their convergence is checked with the results)
    // rank_tiles only.  async: rank_supers_async ran, and its checks (every chain visited, the
    // rounds converged) wait for the starts' scalar read; chain_paths: PK / RK are read through
    // the chains (PathOf over LH / LR) instead of expanded per node
    bool async = false, chain_paths = false;
    unsigned int *LH = nullptr, *LR = nullptr;
};

// rank by tile contraction (rank_tile.h), on minimizer-local ids
template <typename Index>
int rank_tiles(ec_session *s, unsigned int U, const Index &sidx, Ranked &r) {
    hipStream_t st = s->stream;
    const unsigned B = 256;
    Scalars *dsc = s->scal.as<Scalars>();
    const unsigned int N = 2 * U;
    const size_t Nn = std::max<size_t>(N, 1);
    // (1) chains of in-tile links ranked in LDS, in-tile cycles finished (rank_tile.h)
    // tiles cut at bucket starts where the count marked them (k_tile_plan), else fixed
    const bool planned = ids_minimizer_local(sidx) && s->bmark_ok;
    s->bmark_ok = false;
    // (buckets of more than ~300 keys -- config 5's 2^19 tables hold ~376 -- are cut on the
    // finer stride that may round down by up to 512: a cut inside a bucket splits nearly every
    // minimizer run of it, whose k-mers lie in hash order across the bucket's ids)
    const double per_bucket = s->stats.n_buckets ? (double)U / s->stats.n_buckets : 0.0;
    const unsigned int step = per_bucket > 300.0 ? RT_STEP_SEG : RT_STEP;
    const unsigned int ntiles = planned ? (U + step - 1) / step : (N + RT_TN - 1) / RT_TN;
    const unsigned int *tbp = nullptr;
    if (planned) {
        EC_CHECK(s->rt_tb.ensure(((size_t)ntiles + 1) * 4));
        k_tile_plan<<<grid_for(ntiles + 1ull, B), B, 0, st>>>(s->bmark.as<unsigned int>(), U, ntiles,
                                                           s->rt_tb.as<unsigned int>(), 0u, step);
        tbp = s->rt_tb.as<unsigned int>();
    }
    EC_CHECK(s->rt_tcnt.ensure(((size_t)ntiles + 1) * 8));
    EC_CHECK(s->rt_tbase.ensure(((size_t)ntiles + 1) * 8));
    EC_CHECK(s->rt_srec.ensure(Nn * sizeof(SuperRec)));
    EC_CHECK(s->rt_sidx.ensure(Nn * 4));
    EC_CHECK(s->rt_lr.ensure(Nn * 4));
    unsigned int *LH = s->pred.as<unsigned int>(), *LR = s->rt_lr.as<unsigned int>();  // (pred: free here)
    // (a planned tile keeps its chain records at its first node's offset, tb[t] - tb[0]: its
    // chains fit in its nodes, so N records suffice; fixed tiles at scratch[tile * RT_TN ..])
    EC_CHECK(s->st1.ensure(std::max<size_t>(Nn, planned ? 0 : (size_t)ntiles * RT_TN) * sizeof(RJump)));
    SuperRec *scratch = reinterpret_cast<SuperRec *>(s->st1.p);  // (dead before the Wyllie rounds)
    static_assert(sizeof(SuperRec) == sizeof(RJump), "tile scratch in the ruler state buffer");
    unsigned long long *tcnt = s->rt_tcnt.as<unsigned long long>(), *tbase = s->rt_tbase.as<unsigned long long>();
    EC_CHECK(s->rt_hasp.ensure(Nn));  // (sized here: k_tile_compact initialises it for rank_supers)
    // (2) the super list: compacted in tile order, linked, ranked by the weighted ruling set
    // (round 4 measured the same sequence as one cooperative launch: rank stage 0.63 -> 3.3
    // ms, its grid barriers far slower than the launches they replace; removed in round 5)
    unsigned int M = 0;
    r.async = kn().rank_sync != 1;
    r.LH = LH;
    r.LR = LR;
    if (r.async) {  // no read-back: the checks ride on the scalar read after the starts
        // the chains compacted by look-back in k_tile_chains itself (round 6: no scan, no
        // k_tile_compact, LH = super index); the status words are cleared once per allocation
        // (a reallocation is told by the capacity: the new block may come back at the old address)
        const size_t oldcap = s->rt_lb.cap;
        EC_CHECK(s->rt_lb.ensure(((size_t)ntiles + 1) * 8));
        if (s->rt_lb.cap != oldcap) {
            EC_HIP(hipMemsetAsync(s->rt_lb.p, 0, s->rt_lb.cap, st));
            s->lb_epoch = 0;
        }
        s->lb_epoch = (s->lb_epoch + 1) & ((1ull << 30) - 1);
        if (s->lb_epoch == 0) {  // (wrapped: words of 2^30 calls ago could match)
            EC_HIP(hipMemsetAsync(s->rt_lb.p, 0, s->rt_lb.cap, st));
            s->lb_epoch = 1;
        }
        TileLB lb{s->rt_lb.as<unsigned long long>(), s->lb_epoch, s->rt_srec.as<SuperRec>(),
                  s->rt_hasp.as<uint8_t>(), s->rid.as<uint2>(), &dsc->chains, &dsc->nr, &dsc->nvisited};
        k_tile_chains<<<ntiles, RT_NT, 0, st>>>(s->upal.as<uint8_t>(), s->succ.as<unsigned int>(), N,
                                                s->dfc.as<unsigned long long>(), s->dft.as<unsigned long long>(),
                                                LH, LR, tcnt, scratch, s->PK.as<unsigned int>(),
                                                s->RK.as<unsigned int>(), s->PL.as<unsigned int>(),
                                                s->PM.as<unsigned long long>(), 0u, tbp, lb);
        EC_CHECK(rank_supers_async(s, N, &dsc->chains, r.rounds, 0, LH));
        // (3) no k_expand: every reader takes a node's key and rank from its chain (PathOf)
        r.chain_paths = true;
    } else {
        k_tile_chains<<<ntiles, RT_NT, 0, st>>>(s->upal.as<uint8_t>(), s->succ.as<unsigned int>(), N,
                                                s->dfc.as<unsigned long long>(), s->dft.as<unsigned long long>(),
                                                LH, LR, tcnt, scratch, s->PK.as<unsigned int>(),
                                                s->RK.as<unsigned int>(), s->PL.as<unsigned int>(),
                                                s->PM.as<unsigned long long>(), 0u, tbp);
        EC_CHECK(scan_u64(s, tcnt, tbase, (size_t)ntiles + 1));
        // the chain count read back while k_tile_compact (sized by the tiles, not by M) runs:
        // the host's wake-up and next launches overlap the compaction
        unsigned long long M64 = 0;
        if (!s->rd_ev) EC_HIP(hipEventCreateWithFlags(&s->rd_ev, hipEventDisableTiming));
        EC_CHECK(d2h(s, &M64, tbase + ntiles, 8, st));
        EC_HIP(hipEventRecord(s->rd_ev, st));
        k_tile_compact<<<ntiles, 256, 0, st>>>(scratch, tcnt, tbase, s->rt_srec.as<SuperRec>(),
                                               s->rt_sidx.as<unsigned int>(), s->rt_hasp.as<uint8_t>(),
                                               s->rid.as<uint2>(), &dsc->nr, &dsc->nvisited, nullptr, tbp);
        EC_CHECK(host_wait(s, s->rd_ev));
        M = (unsigned int)M64;
    }
    if (!r.async && M) {
        EC_CHECK(rank_supers(s, M, N, r.nr, r.rounds, true));
        // (3) every node: its chain's key and rank + its offset in the chain
        k_expand<<<grid_for(N, B), B, 0, st>>>(LH, LR, N, s->rt_sidx.as<unsigned int>(), s->rt_pks.as<unsigned int>(),
                                              s->rt_rks.as<unsigned int>(), s->PK.as<unsigned int>(),
                                              s->RK.as<unsigned int>());
    }
    return EC_OK;
}

// rank by the node-level ruling set: up to four host-checked ruler passes, weighted Wyllie on the
// rulers
int rank_nodes(ec_session *s, unsigned int U, unsigned int &nr, int &rounds) {
    hipStream_t st = s->stream;
    const unsigned B = 256;
    Scalars *dsc = s->scal.as<Scalars>();
    const unsigned int N = 2 * U;
    const size_t Nn = std::max<size_t>(N, 1);
    Scalars hsc{};
    EC_HIP(hipMemsetAsync(s->rid.p, 0xFF, Nn * 8, st));
    EC_CHECK(s->nrec.ensure(Nn * sizeof(NodeRec)));
    unsigned int masks[4] = {31u, 7u, 1u, 0u};
    unsigned int r0 = 0;
    for (int it = 0; it < 4; it++) {
        const unsigned int nblk = (unsigned int)((N + RULER_CHUNK - 1) / RULER_CHUNK);
        if (it)  // (it = 0: counted by k_pred_rc with masks[0])
            k_rulers_count<<<nblk, B, 0, st>>>(s->upal.as<uint8_t>(), s->pred.as<unsigned int>(), N, masks[it],
                                               it == 0, s->rid.as<uint2>(), s->rbc.as<unsigned int>());
        EC_CHECK(scan_incl_u32(s, s->rbc.as<unsigned int>(), s->rbc.as<unsigned int>() + nblk, nblk));
        k_rulers<<<nblk, B, 0, st>>>(s->upal.as<uint8_t>(), s->pred.as<unsigned int>(), N, masks[it], it == 0,
                                     s->rbc.as<unsigned int>() + nblk, &dsc->nr, s->rid.as<uint2>(),
                                     s->rlist.as<unsigned int>(),
                                     it == 0 ? s->outdeg.as<unsigned long long>() : nullptr);
        k_rulers_total<<<1, 1, 0, st>>>(s->rbc.as<unsigned int>() + nblk, nblk, &dsc->nr);
        k_walk<<<2048, B, 0, st>>>(s->nrec.as<NodeRec>(), s->rlist.as<unsigned int>(), r0, &dsc->nr,
                                  masks[it], s->rid.as<uint2>(),
                                  s->nextR.as<unsigned int>(), s->st0.as<RJump>(), &dsc->nvisited);
        EC_CHECK(d2h(s, &hsc, dsc, sizeof(Scalars), st));
        EC_CHECK(host_sync(s, st));
        r0 = hsc.nr;
        if (hsc.nvisited + hsc.npal >= N) break;
    }
    nr = hsc.nr;
    if (hsc.nvisited + hsc.npal != N) {
        set_error("ruling set covered %llu of %u nodes", (unsigned long long)(hsc.nvisited + hsc.npal), N);
        return EC_ERR_STATE;
    }
    k_rjump_init<<<grid_for(nr, B), B, 0, st>>>(s->nextR.as<unsigned int>(), nr, s->st0.as<RJump>());
    rounds = 1;
    while ((1ull << (rounds - 1)) < (unsigned long long)nr) rounds++;
    rounds = std::min(rounds + 1, 63);
    RJump *bufs[2] = {s->st0.as<RJump>(), s->st1.as<RJump>()};
    for (int r = 0; r < rounds; r++)
        k_rjump<<<grid_for(nr, B), B, 0, st>>>(bufs[r & 1], bufs[(r + 1) & 1], nr, N,
                                              r ? &dsc->active[r - 1] : nullptr, &dsc->active[r],
                                              &dsc->final_sel, (unsigned)((r + 1) & 1));
    k_finalize<<<grid_for(N, B), B, 0, st>>>(s->upal.as<uint8_t>(), s->succ.as<unsigned int>(),
                                            s->rid.as<uint2>(), s->rlist.as<unsigned int>(), bufs[0], bufs[1],
                                            &dsc->final_sel, &dsc->active[rounds - 1], N, s->PK.as<unsigned int>(),
                                            s->RK.as<unsigned int>(), s->PL.as<unsigned int>(),
                                            s->PM.as<unsigned long long>());
    k_cycle_len<<<grid_for(nr, B), B, 0, st>>>(s->nextR.as<unsigned int>(), s->rlist.as<unsigned int>(), bufs[0],
                                              bufs[1], &dsc->final_sel, &dsc->active[rounds - 1], nr,
                                              s->PL.as<unsigned int>(),
                                              s->PM.as<unsigned long long>());
    return EC_OK;
}

// the contig starts (nodes with their component's smallest first event) as sort pairs, and the
// scalars read back (hsc: nstarts, active[], the chain count) while the emission's node maps are
// cleared; run again after the ranking had to be redone
int starts_pass(ec_session *s, unsigned int U, const PathOf &P, unsigned int nx, Scalars &hsc) {
    hipStream_t st = s->stream;
    const unsigned B = 256;
    Scalars *dsc = s->scal.as<Scalars>();
    const unsigned int N = 2 * U;
    const size_t Nn = std::max<size_t>(N, 1);
    if (U) {
        const unsigned int nblk = (unsigned int)((N + RULER_CHUNK - 1) / RULER_CHUNK);
        unsigned int *bc = s->rbc.as<unsigned int>(), *bs = bc + nblk;
        // the start bits between the two passes live in `cand` (free after the links)
        EC_CHECK(s->cand.ensure(std::max<size_t>(Nn * 4, (Nn / 64 + 8) * 8)));
        unsigned long long *smask = s->cand.as<unsigned long long>();
        k_starts_count<<<nblk, B, 0, st>>>(s->upal.as<uint8_t>(), s->dfc.as<unsigned long long>(),
                                           s->dft.as<unsigned long long>(), P,
                                           s->PM.as<unsigned long long>(), N, bc, smask,
                                           nx ? s->x_in.as<uint8_t>() : nullptr);
        EC_CHECK(scan_incl_u32(s, bc, bs, nblk));
        k_starts_write<<<nblk, B, 0, st>>>(s->upal.as<uint8_t>(), s->dfc.as<unsigned long long>(),
                                           s->dft.as<unsigned long long>(), P,
                                           s->PM.as<unsigned long long>(), N, bs, smask,
                                           s->skeys.as<unsigned long long>(), s->svals.as<unsigned int>(), 0u,
                                           &dsc->nstarts);
    }
    EC_CHECK(d2h(s, &hsc, dsc, sizeof(Scalars), st));  // nstarts, active[], the chain count
    if (!s->rd_ev) EC_HIP(hipEventCreateWithFlags(&s->rd_ev, hipEventDisableTiming));
    EC_HIP(hipEventRecord(s->rd_ev, st));
    // (skew: k_emit raises it at a position past the character bound)
    k_emit_init<<<grid_for(Nn / 4 + 1, B, 2048), B, 0, st>>>(s->headOf.as<unsigned int>(), s->tailOf.as<unsigned int>(),
                                                            s->cidxOf.as<unsigned int>(), Nn, &dsc->skew);
    EC_CHECK(host_wait(s, s->rd_ev));
    return EC_OK;
}

// the output stream and its events (ec_session::oev), created on first use
int ostream_ready(ec_session *s) {
    if (!s->ostream) EC_HIP(hipStreamCreateWithFlags(&s->ostream, hipStreamNonBlocking));
    for (auto &e : s->oev)
        if (!e) EC_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return EC_OK;
}

// host bytes of n contig characters (packed: 2-bit codes, 4 a byte)
inline uint64_t char_bytes(bool pack, uint64_t n) { return pack ? (n + 3) / 4 : n; }

// results to host (links compacted on the device: only the used entries travel): the link
// counts, offsets and total -- few contigs: one block with the contig offsets -- the bound checks
// on the characters, then what the first round trip sized: characters past the early copy's pre
// (from csrc, packed or not) and the compacted links
int results_to_host(ec_session *s, unsigned int nc, bool small, bool ocopy, uint64_t chars_bound, bool pack,
                    const void *csrc, uint64_t pre) {
    hipStream_t st = s->stream;
    const unsigned B = 256;
    Scalars *dsc = s->scal.as<Scalars>();
    const unsigned int n2 = 2 * nc;
    s->links_compact = true;
    EC_CHECK(s->h_lc8.resize(n2));
    if (!nc) s->h_coff[0] = 0;
    if (nc && !ocopy && !small) EC_CHECK(d2h(s, s->h_coff.data(), s->coff.p, (size_t)nc * 8, st));
    unsigned long long nlinks64 = 0;
    unsigned int emit_bad = 0;
    // the small path's result block: [link total u64][emission flag u32, pad][contig offsets
    // (nc + 1) u64][links 8 n2 u32 (their bound)][link counts n2 bytes]
    const size_t blk_coff = 16, blk_links = blk_coff + ((size_t)nc + 1) * 8, blk_lc8 = blk_links + (size_t)n2 * 8 * 4,
                 blk_bytes = blk_lc8 + n2;
    if (nc && small) {
        // (n2 <= 8192: counts, offsets and the compacted links in one launch; the links' bound
        // 8 n2 travels with the total, so no second round trip follows -- and with them the contig
        // offsets and the emission's flag: one copy where six 4-5 us copies stood in a row)
        EC_CHECK(s->dcounts.ensure(blk_bytes));
        EC_CHECK(s->h_blk.resize(blk_bytes));
        char *blk = s->dcounts.as<char>();
        k_links_small<<<1, SMALL_LINK_NT, 0, st>>>(
            s->lk.as<long long>(), s->lcnt.as<unsigned int>(), n2, reinterpret_cast<uint8_t *>(blk + blk_lc8),
            reinterpret_cast<uint32_t *>(blk + blk_links), reinterpret_cast<unsigned long long *>(blk),
            s->coff.as<unsigned long long>(), nc + 1, reinterpret_cast<unsigned long long *>(blk + blk_coff),
            &dsc->skew, reinterpret_cast<unsigned int *>(blk + 8));
        EC_CHECK(d2h(s, s->h_blk.data(), blk, blk_bytes, st));
    } else if (nc) {
        EC_CHECK(s->skeys.ensure(((size_t)n2 + 1) * 8));   // per-side counts as u64 (starts sorted)
        EC_CHECK(s->skeys2.ensure(((size_t)n2 + 1) * 8));  // their exclusive scan = link offsets
        // (the counts as bytes in a buffer of their own: the scan's temporary storage is s->tmp)
        EC_CHECK(s->lc8.ensure(n2));
        k_lcnt64<<<grid_for(n2 + 1ull, B), B, 0, st>>>(s->lcnt.as<unsigned int>(), n2, s->skeys.as<unsigned long long>(),
                                                       s->lc8.as<uint8_t>());
        if (ocopy) {
            EC_HIP(hipEventRecord(s->oev[3], st));
            EC_HIP(hipStreamWaitEvent(s->ostream, s->oev[3], 0));
            EC_HIP(hipMemcpyAsync(s->h_lc8.data(), s->lc8.p, n2, hipMemcpyDeviceToHost, s->ostream));
        } else {
            EC_CHECK(d2h(s, s->h_lc8.data(), s->lc8.p, n2, st));
        }
        EC_CHECK(scan_u64(s, s->skeys.as<unsigned long long>(), s->skeys2.as<unsigned long long>(), (size_t)n2 + 1));
        EC_CHECK(d2h(s, &nlinks64, s->skeys2.as<unsigned long long>() + n2, 8, st));
    }
    if (!(nc && small)) EC_CHECK(d2h(s, &emit_bad, &dsc->skew, 4, st));
    EC_CHECK(host_sync(s, st));  // h_coff[nc] (the characters), the link total
    if (nc && small) {
        const char *hb = s->h_blk.data();
        std::memcpy(&nlinks64, hb, 8);
        std::memcpy(&emit_bad, hb + 8, 4);
        std::memcpy(s->h_coff.data(), hb + blk_coff, ((size_t)nc + 1) * 8);
        std::memcpy(s->h_lc8.data(), hb + blk_lc8, n2);
        nlinks64 = std::min<unsigned long long>(nlinks64, (unsigned long long)n2 * 8);
        EC_CHECK(s->h_links32.resize(nlinks64));
        std::memcpy(s->h_links32.data(), hb + blk_links, (size_t)nlinks64 * 4);
    }
    const uint64_t nchars = s->h_coff[nc];
    if (emit_bad || nchars > chars_bound) EC_HIP(hipStreamSynchronize(s->ostream));  // (no copy left in flight)
    if (emit_bad) {
        set_error("contig characters past their bound %llu (inconsistent ranking)", (unsigned long long)chars_bound);
        return EC_ERR_STATE;
    }
    s->stats.n_contig_chars = nchars;
    if (nchars > chars_bound) {
        set_error("contig characters %llu past their bound %llu", (unsigned long long)nchars,
                  (unsigned long long)chars_bound);
        return EC_ERR_STATE;
    }
    if (pre && nchars > pre) EC_HIP(hipEventSynchronize(s->oev[1]));  // (before h_chars may move)
    EC_CHECK(s->h_chars.resize(char_bytes(pack, nchars)));
    s->chars_packed = pack;
    s->nchars_host = nchars;
    bool again = nchars > pre;  // (a second round trip: characters or links still to copy)
    if (nchars > pre) EC_CHECK(d2h(s, s->h_chars.data(), csrc, char_bytes(pack, nchars), st));
    const uint64_t nlinks = nlinks64;
    EC_CHECK(s->h_links32.resize(nlinks));  // (small: the copied bound's first nlinks stay)
    if (nlinks && !small) {
        again = true;
        EC_CHECK(s->dcounts.ensure(nlinks * 4));
        k_links_compact<uint32_t><<<grid_for(n2, B), B, 0, st>>>(s->lk.as<long long>(), s->lcnt.as<unsigned int>(),
                                                                s->skeys2.as<unsigned long long>(), n2,
                                                                s->dcounts.as<uint32_t>());
        EC_CHECK(d2h(s, s->h_links32.data(), s->dcounts.p, nlinks * 4, st));
    }
    if (again) EC_CHECK(host_sync(s, st));
    if (ocopy || pre) EC_HIP(hipStreamSynchronize(s->ostream));  // (offsets, characters, link counts)
    s->last_nchars = nchars;
    s->stats.n_links = nlinks;
    return EC_OK;
}

// all_contigs:79-111 on the device from the solid set of phase_count / phase_merge
template <typename Ops, typename Index>
int phase_graph(ec_session *s, int k, unsigned int U, const Index &sidx, const unsigned int *ext_succ = nullptr) {
    hipStream_t st = s->stream;
    const unsigned B = 256;
    Scalars *dsc = s->scal.as<Scalars>();
    Scalars hsc{};
    const unsigned int N = 2 * U;
    const size_t Nn = std::max<size_t>(N, 1);
    // list ranking by tile contraction (rank_tile.h) on minimizer-local ids, the node-level
    // ruling set otherwise (EULERHIP_RANK=1 / 2 force one or the other); tile ranking needs
    // neither pred nor the node walk records
    const bool tile_rank = kn().rank == 2 || (kn().rank != 1 && ids_minimizer_local(sidx));
    constexpr bool XT = std::is_same<Ops, OpsX>::value;  // extended alphabet (extended.h)

    // ---- links ----------------------------------------------------------------------------
    mark(s, 2 * EC_STAGE_LINKS);
    unsigned int nx = 0;  // extended alphabet: dict entries of components with one-way links
    EC_CHECK((graph_links<Ops, Index>(s, k, U, sidx, ext_succ, tile_rank, nx)));
    mark(s, 2 * EC_STAGE_LINKS + 1);

    // ---- rank (sparse ruling set + weighted Wyllie on the rulers) -------------------------
    mark(s, 2 * EC_STAGE_RANK);
    EC_CHECK(s->rid.ensure(Nn * 8));  // (ruler, offset) per node
    EC_CHECK(s->rlist.ensure(Nn * 4));
    EC_CHECK(s->rbc.ensure(((Nn + RULER_CHUNK - 1) / RULER_CHUNK) * 8));
    EC_CHECK(s->nextR.ensure(Nn * 4));
    EC_CHECK(s->st0.ensure(Nn * sizeof(RJump)));
    EC_CHECK(s->st1.ensure(Nn * sizeof(RJump)));
    EC_CHECK(s->PK.ensure(Nn * 4));
    EC_CHECK(s->RK.ensure(Nn * 4));
    EC_CHECK(s->PL.ensure(Nn * 4));
    EC_CHECK(s->PM.ensure(Nn * 8));
    Ranked rk;
    s->stats.rank_rounds = 0;
    if (U && tile_rank) EC_CHECK(rank_tiles(s, U, sidx, rk));
    if (U && !tile_rank) EC_CHECK(rank_nodes(s, U, rk.nr, rk.rounds));
    s->stats.n_rulers = rk.nr;
    mark(s, 2 * EC_STAGE_RANK + 1);

    // ---- starts + order -------------------------------------------------------------------
    const PathOf P = rk.chain_paths ? PathOf{s->PK.as<unsigned int>(), s->RK.as<unsigned int>(), rk.LH, rk.LR,
                                             s->rt_pks.as<unsigned int>(), s->rt_rks.as<unsigned int>()}
                                    : path_of(s->PK.as<unsigned int>(), s->RK.as<unsigned int>());
    mark(s, 2 * EC_STAGE_STARTS);
    EC_CHECK(s->cidxOf.ensure(Nn * 4));
    EC_CHECK(s->skeys.ensure(Nn * 8));
    EC_CHECK(s->svals.ensure(Nn * 4));
    EC_CHECK(s->skeys2.ensure(Nn * 8));
    EC_CHECK(s->svals2.ensure(Nn * 4));
    // the emission's node maps are cleared behind the starts' read-back copy (below): the device
    // works through the fills while the host wakes up; the start kernels read none of them
    EC_CHECK(s->headOf.ensure(Nn * 4));
    EC_CHECK(s->tailOf.ensure(Nn * 4));
    EC_CHECK(starts_pass(s, U, P, nx, hsc));
    if (rk.async) {  // the asynchronous ranking's checks, on the scalars the starts read back
        const unsigned int Ma = (unsigned int)hsc.chains;
        rk.nr = hsc.nr;
        s->stats.n_rulers = rk.nr;
        if (kn().verbose)
            fprintf(stderr, "rank: %u oriented nodes, %u chains (tile contraction), %u rulers, %llu visited\n", N, Ma,
                    rk.nr, (unsigned long long)hsc.nvisited);
        if (Ma) note_rounds(s, hsc, rk.rounds);
        if (hsc.nvisited != Ma || (Ma && hsc.active[rk.rounds - 1] != 0)) {
            // a cycle of chains no ruler reached (or unconverged rounds): the ranking with its
            // host-checked ruler passes, then the starts again
            if (kn().verbose)
                fprintf(stderr, "rank: one ruler pass covered %llu of %u chains, ranking again\n",
                        (unsigned long long)hsc.nvisited, Ma);
            rk.async = false;
            // (the look-back compaction's LH: super index per node, at heads the head -> index map)
            EC_CHECK(rank_supers(s, Ma, N, rk.nr, rk.rounds, false, rk.LH));  // (PathOf reads the new PKs / RKs)
            s->stats.n_rulers = rk.nr;
            EC_CHECK(starts_pass(s, U, P, nx, hsc));
        }
    }
    if (rk.rounds) {
        unsigned int used = 1;
        for (int r = 0; r < rk.rounds; r++)
            if (hsc.active[r]) used = r + 2;
        s->stats.rank_rounds = std::min<unsigned int>(used, rk.rounds);
        if (hsc.active[rk.rounds - 1] != 0) {
            set_error("ruler list ranking did not converge in %d rounds", rk.rounds);
            return EC_ERR_STATE;
        }
    }
    unsigned int nc = hsc.nstarts;
    unsigned int nsort = nc;
    if (nx) {  // all_contigs on the components with one-way links, their starts after the others
        EC_CHECK(s->x_done.ensure(Nn));
        EC_CHECK(s->x_len.ensure((size_t)nx * 4));
        EC_CHECK(s->x_m.ensure((size_t)nx * 4));
        EC_CHECK(s->x_cid.ensure((size_t)nx * 4));
        EC_HIP(hipMemsetAsync(s->x_done.p, 0, Nn, st));
        k_x_emulate<<<grid_for(nx, 64), 64, 0, st>>>(
            s->x_lv.as<unsigned int>(), nx, s->x_par.as<unsigned int>(), s->upal.as<uint8_t>(),
            s->x_succ.as<unsigned int>(), s->dkey.as<K128>(), k, N, s->dfc.as<unsigned long long>(),
            s->dft.as<unsigned long long>(), s->x_done.as<uint8_t>(), s->skeys.as<unsigned long long>() + nc,
            s->svals.as<unsigned int>() + nc, s->x_len.as<unsigned int>(), s->x_m.as<unsigned int>(), &dsc->nxs,
            &dsc->xbad);
        unsigned int xs[2] = {0, 0};
        EC_CHECK(d2h(s, xs, &dsc->nxs, 8, st));
        EC_CHECK(host_sync(s, st));
        if (xs[1]) {
            set_error("a contig walk enters a cycle without its start: the reference's get_contig_forward "
                      "(referenceAssembler.py:59-77) never returns on this input");
            return EC_ERR_STATE;
        }
        nsort = nc + nx;  // (the emulation's non-starts carry key NONE: sorted past the starts)
        nc += xs[0];
    }
    s->stats.n_contigs = nc;
    EC_CHECK(s->cwalk.ensure((size_t)std::max(nc, 1u) * sizeof(Walk)));
    EC_CHECK(s->coff.ensure((size_t)(nc + 1) * 8));
    EC_CHECK(s->ewalk.ensure((size_t)std::max(nc, 1u) * sizeof(EWalk)));
    // few starts: order, walks, offsets and emission records in one workgroup (k_starts_small)
    const bool small = !nx && nc && nc <= SMALL_STARTS && !kn().no_small_starts;
    if (small)
        k_starts_small<<<1, SMALL_STARTS_NT, 0, st>>>(
            s->skeys.as<unsigned long long>(), s->svals.as<unsigned int>(), nc, s->upal.as<uint8_t>(),
            P, s->PL.as<unsigned int>(), k,
            s->svals2.as<unsigned int>(), s->cidxOf.as<unsigned int>(), s->coff.as<unsigned long long>(),
            s->cwalk.as<Walk>(), s->ewalk.as<EWalk>());
    if (nsort && !small)
        EC_CHECK(sort_pairs(s, s->skeys.as<unsigned long long>(), s->skeys2.as<unsigned long long>(),
                            s->svals.as<unsigned int>(), s->svals2.as<unsigned int>(), nsort));
    const unsigned int *sorted_nodes = s->svals2.as<unsigned int>();
    if (!small) {
        EC_CHECK(s->clen.ensure((size_t)(nc + 1) * 8));
        EC_HIP(hipMemsetAsync(s->clen.p, 0, (size_t)(nc + 1) * 8, st));
        if (nc)
            k_contig_len<<<grid_for(nc, B), B, 0, st>>>(
                s->upal.as<uint8_t>(), P, s->PL.as<unsigned int>(), sorted_nodes, nc, k, s->cidxOf.as<unsigned int>(),
                s->clen.as<unsigned long long>(), s->cwalk.as<Walk>(), nx ? s->x_len.as<unsigned int>() : nullptr,
                nx ? s->x_cid.as<unsigned int>() : nullptr);
        EC_CHECK(scan_u64(s, s->clen.as<unsigned long long>(), s->coff.as<unsigned long long>(), nc + 1));
    }
    // the total travels with the other results (no round trip here): the character buffer is
    // sized for the bound 2U + nc (k - 1) (a walk covers at most its path; a self-twin path's
    // nodes are up to twice its canonical k-mers)
    // (few contigs: k_links_small's result block carries the offsets and the total)
    EC_CHECK(s->h_coff.resize(nc + 1));
    if (!small) EC_CHECK(d2h(s, &s->h_coff[nc], s->coff.as<unsigned long long>() + nc, 8, st));
    // the results' copies to host memory run on the output stream, each as soon as its data is
    // final: the contig offsets here (overlapping emission and GFA), the characters after the
    // emission, the link offsets after the GFA counts (ecoli10m_err: 1.1 M contigs, 47 MB of
    // results copied after GFA took ~1 ms in line)
    // (only for many contigs: the event / stream-wait / copy calls cost the host ~30 us, more
    // than the headline's few bytes of offsets and link counts take in line)
    const bool ocopy = nc >= OCOPY_MIN;
    EC_CHECK(ostream_ready(s));
    if (ocopy) {
        EC_HIP(hipEventRecord(s->oev[2], st));
        EC_HIP(hipStreamWaitEvent(s->ostream, s->oev[2], 0));
        EC_HIP(hipMemcpyAsync(s->h_coff.data(), s->coff.p, (size_t)nc * 8, hipMemcpyDeviceToHost, s->ostream));
    }
    mark(s, 2 * EC_STAGE_STARTS + 1);
    uint64_t chars_bound = 2ull * U + (uint64_t)nc * (uint64_t)(k - 1);
    if (nx) {  // emulated contigs may overlap: the bound is their exact total
        unsigned long long tot = 0;
        EC_CHECK(d2h(s, &tot, s->coff.as<unsigned long long>() + nc, 8, st));
        EC_CHECK(host_sync(s, st));
        chars_bound = std::max<uint64_t>(chars_bound, tot);
    }

    // ---- emit -----------------------------------------------------------------------------
    mark(s, 2 * EC_STAGE_EMIT);
    EC_CHECK(s->chars.ensure(std::max<size_t>(chars_bound, 1) + 16));  // (+16: k_pack_chars reads 16 at a time)
    EC_CHECK(s->cfirst.ensure((size_t)std::max(nc, 1u) * 4));
    EC_CHECK(s->clast.ensure((size_t)std::max(nc, 1u) * 4));
    if (nc && !small)
        k_ewalk<<<grid_for(nc, B), B, 0, st>>>(s->cwalk.as<Walk>(), s->coff.as<unsigned long long>(), nc,
                                              s->ewalk.as<EWalk>());
    if (U)
        k_emit<Ops><<<grid_for(N, B), B, 0, st>>>(s->upal.as<uint8_t>(), P,
                                            s->PL.as<unsigned int>(), s->dkey.as<typename Ops::K>(),
                                            s->cidxOf.as<unsigned int>(), s->ewalk.as<EWalk>(),
                                            N, k, s->chars.as<char>(), std::max<uint64_t>(chars_bound, 1),
                                            s->cfirst.as<unsigned int>(), s->clast.as<unsigned int>(),
                                            s->headOf.as<unsigned int>(), s->tailOf.as<unsigned int>(), &dsc->skew);
    if constexpr (XT) {
        if (nx) {
            EC_CHECK(s->x_head.ensure(Nn * 4));
            EC_CHECK(s->x_tail.ensure(Nn * 4));
            EC_HIP(hipMemsetAsync(s->x_head.p, 0, Nn * 4, st));
            EC_HIP(hipMemsetAsync(s->x_tail.p, 0, Nn * 4, st));
            k_x_emit<<<grid_for(nx, B), B, 0, st>>>(
                s->x_lv.as<unsigned int>(), s->x_len.as<unsigned int>(), s->x_m.as<unsigned int>(),
                s->x_cid.as<unsigned int>(), s->skeys.as<unsigned long long>() + hsc.nstarts, nx, s->upal.as<uint8_t>(),
                s->x_succ.as<unsigned int>(), s->dkey.as<K128>(), k, s->coff.as<unsigned long long>(),
                s->chars.as<char>(), s->cfirst.as<unsigned int>(), s->clast.as<unsigned int>(),
                s->x_head.as<unsigned int>(), s->x_tail.as<unsigned int>());
            k_x_heads<<<grid_for(N, B), B, 0, st>>>(N, s->x_head.as<unsigned int>(), s->x_tail.as<unsigned int>(),
                                                    s->headOf.as<unsigned int>(), s->tailOf.as<unsigned int>());
        }
    }
    // the characters' copy to host memory starts on the output stream as soon as the emission is
    // done, sized by the previous call's total (a stream of equal batches, the bench's steps): it
    // overlaps GFA and the link compaction instead of following a read-back of the total; a
    // larger total is copied again in full after the read-back
    // standard alphabet: the characters travel as 2-bit codes (a quarter of the PCIe bytes)
    const bool pack = !XT && kn().no_char_pack == 0;
    const void *csrc = s->chars.p;
    if (pack) {
        const uint64_t cap16 = (std::max<uint64_t>(chars_bound, 1) + 15) / 16;
        EC_CHECK(s->dchars.ensure(cap16 * 4));
        k_pack_chars<<<std::min(grid_for(cap16, B), 8192u), B, 0, st>>>(
            s->chars.as<uint4>(), s->coff.as<unsigned long long>() + nc, cap16, s->dchars.as<uint32_t>());
        csrc = s->dchars.p;
    }
    uint64_t pre = 0;
    if (s->last_nchars && s->last_nchars <= chars_bound && kn().no_spec == 0) {
        pre = s->last_nchars;
        EC_CHECK(s->h_chars.resize(char_bytes(pack, pre)));
        EC_HIP(hipEventRecord(s->oev[0], st));
        EC_HIP(hipStreamWaitEvent(s->ostream, s->oev[0], 0));
        EC_HIP(hipMemcpyAsync(s->h_chars.data(), csrc, char_bytes(pack, pre), hipMemcpyDeviceToHost, s->ostream));
        EC_HIP(hipEventRecord(s->oev[1], s->ostream));
    }
    s->last_nchars = 0;
    mark(s, 2 * EC_STAGE_EMIT + 1);

    // ---- GFA ------------------------------------------------------------------------------
    mark(s, 2 * EC_STAGE_GFA);
    EC_CHECK(s->lk.ensure((size_t)std::max(nc, 1u) * 16 * 8));
    EC_CHECK(s->lcnt.ensure((size_t)std::max(nc, 1u) * 2 * 4));
    if (nc)
        k_gfa<Ops, Index><<<grid_for(nc, B), B, 0, st>>>(sidx, s->dkey.as<typename Ops::K>(),
                                            s->upal.as<uint8_t>(), s->cfirst.as<unsigned int>(),
                                            s->clast.as<unsigned int>(), s->headOf.as<unsigned int>(),
                                            s->tailOf.as<unsigned int>(), nc, k, s->lk.as<long long>(),
                                            s->lcnt.as<unsigned int>());
    mark(s, 2 * EC_STAGE_GFA + 1);

    // ---- results to host -------------------------------------------------------------------
    EC_CHECK(results_to_host(s, nc, small, ocopy, chars_bound, pack, csrc, pre));

    s->stats.n_dict = 2ull * U - hsc.npal;  // len(build()): palindromes have one entry

    collect_timing(s);
    s->have = true;
    s->stats_ok = true;
    // ec_clip_tips works on what this phase leaves: the dense arrays with the index k_gfa just
    // read, chars / coff, lk / lcnt -- of a complete set (no partitioned links) on A/C/G/T
    if (XT) s->clip_why = "the results are on an extended alphabet";
    else if (ext_succ) s->clip_why = CLIP_WHY_STEPWISE;
    else {
        keep_index(s, sidx);
        s->clip_ok = true;
    }
    return EC_OK;
}

// ---- multi-GPU partitioned finish (distributed.py): each rank ranks and emits its own segment --
// of the loaded (gathered) solid set, canonical ids [lo, hi) = oriented nodes [n0, n1):
//   ec_graph_chains_part  its links' chains ranked in LDS (rank_tile.h) -> its super records
//   ec_graph_rank_supers  every rank: the job's super list (all-gathered, rank order) ranked
//   ec_graph_starts_part  its nodes' keys / ranks, its contig starts -> start records
//   ec_graph_layout       every rank: the job's starts (all-gathered) in event order, offsets
//   ec_graph_emit_part    its nodes' characters at their global positions, its contig ends
//   ec_graph_collect      rank 0: the summed characters / ends -> GFA links and the results
// the chain records of k_tile_chains compacted into d_super (M of them)
int part_chains_copy(ec_session *s, uint64_t M, unsigned int ntiles, bool planned, SuperRec *d_super) {
    if (!s->chain_scr) {  // (the tile records' buffer was released or rewritten since ec_graph_chains_part)
        set_error("ec_graph_chains_copy: the chain records are gone");
        return EC_ERR_STATE;
    }
    hipStream_t st = s->stream;
    if (M)
        k_tile_compact<<<ntiles, 256, 0, st>>>(s->chain_scr, s->rt_tcnt.as<unsigned long long>(),
                                               s->rt_tbase.as<unsigned long long>(), d_super,
                                               s->rt_sidx.as<unsigned int>(), nullptr, nullptr, nullptr, nullptr,
                                               nullptr, planned ? s->rt_tb.as<unsigned int>() : nullptr);
    EC_CHECK(host_sync(s, st));
    return EC_OK;
}

template <typename Ops>
int part_chains(ec_session *s, uint64_t lo, uint64_t hi, const uint32_t *d_succ, SuperRec *d_super,
                uint64_t *n_super) {
    hipStream_t st = s->stream;
    const unsigned B = 256;
    Scalars *dsc = s->scal.as<Scalars>();
    const unsigned int U = (unsigned int)s->n_dense, N = 2 * U;
    const size_t Nn = std::max<size_t>(N, 1);
    const unsigned int n0 = (unsigned int)(2 * lo), n1 = (unsigned int)(2 * hi);
    // (the chains are ranked anew: held records, emitted runs and later steps of an earlier
    // ranking are stale -- their buffers are rewritten below)
    drop_step_state(s);
    EC_CHECK(s->upal.ensure(std::max<size_t>(U, 1)));
    EC_CHECK(s->succ.ensure(Nn * 4));
    EC_CHECK(s->PK.ensure(Nn * 4));
    EC_CHECK(s->RK.ensure(Nn * 4));
    EC_CHECK(s->PL.ensure(Nn * 4));
    EC_CHECK(s->PM.ensure(Nn * 8));
    EC_CHECK(s->pred.ensure(Nn * 4));
    EC_CHECK(s->rt_lr.ensure(Nn * 4));
    EC_CHECK(s->rt_sidx.ensure(Nn * 4));
    if (!s->placed) {  // (a placed segment has its flags and links already: ec_graph_place / join)
        EC_HIP(hipMemsetAsync(&dsc->npal, 0, 4, st));
        EC_CHECK(launch_upal<Ops>(st, s->dkey.as<typename Ops::K>(), U, s->k, s->upal.as<uint8_t>(), &dsc->npal));
    }
    if (n1 > n0 && d_succ)
        EC_HIP(hipMemcpyAsync(s->succ.as<unsigned int>() + n0, d_succ, (size_t)(n1 - n0) * 4, hipMemcpyDeviceToDevice,
                              st));
    // tiles cut at the bucket starts this rank's owner merge marked (its output is this segment)
    const bool planned = s->seg_marks && s->seg_marks == hi - lo && hi > lo;
    const unsigned int ntiles =
        planned ? (unsigned int)((hi - lo + RT_STEP_SEG - 1) / RT_STEP_SEG) : (n1 - n0 + RT_TN - 1) / RT_TN;
    const unsigned int *tbp = nullptr;
    if (planned) {
        EC_CHECK(s->rt_tb.ensure(((size_t)ntiles + 1) * 4));
        k_tile_plan<<<grid_for(ntiles + 1ull, B), B, 0, st>>>(s->bmark.as<unsigned int>(), (unsigned int)(hi - lo),
                                                           ntiles, s->rt_tb.as<unsigned int>(), (unsigned int)lo,
                                                           RT_STEP_SEG);
        tbp = s->rt_tb.as<unsigned int>();
    }
    EC_CHECK(s->rt_tcnt.ensure(((size_t)ntiles + 1) * 8));
    EC_CHECK(s->rt_tbase.ensure(((size_t)ntiles + 1) * 8));
    // (planned tiles keep their chain records at node offsets: 2 (hi - lo) records.)  A placed
    // segment's junction slots (4 a key of >= 16 B: >= the 64 B a key of chain records) are free
    // once ec_graph_place_copy gathered them, so the records go there instead of a buffer of
    // their own (12.6 GB at one config-5 rank); the pending place records are dropped with them
    const size_t scr_bytes =
        std::max<size_t>(planned ? 2 * (size_t)(hi - lo) : (size_t)ntiles * RT_TN, 1) * sizeof(SuperRec);
    DevBuf &scr = s->placed && s->jrec.cap >= scr_bytes ? s->jrec : s->st1;
    EC_CHECK(scr.ensure(scr_bytes));
    unsigned long long *tcnt = s->rt_tcnt.as<unsigned long long>(), *tbase = s->rt_tbase.as<unsigned long long>();
    SuperRec *scratch = reinterpret_cast<SuperRec *>(scr.p);
    s->chain_scr = scratch;
    if (!ntiles) EC_HIP(hipMemsetAsync(tcnt, 0, 8, st));  // (k_tile_chains zeroes tcnt[ntiles])
    if (ntiles)
        k_tile_chains<<<ntiles, RT_NT, 0, st>>>(s->upal.as<uint8_t>(), s->succ.as<unsigned int>(), n1,
                                                s->dfc.as<unsigned long long>(), s->dft.as<unsigned long long>(),
                                                s->pred.as<unsigned int>(), s->rt_lr.as<unsigned int>(), tcnt, scratch,
                                                s->PK.as<unsigned int>(), s->RK.as<unsigned int>(),
                                                s->PL.as<unsigned int>(), s->PM.as<unsigned long long>(), n0, tbp);
    EC_CHECK(scan_u64(s, tcnt, tbase, (size_t)ntiles + 1));
    unsigned long long M = 0;
    EC_CHECK(d2h(s, &M, tbase + ntiles, 8, st));
    EC_CHECK(host_sync(s, st));
    *n_super = M;
    s->seg_n0 = n0;
    s->seg_n1 = n1;
    s->part_stage = 1;
    if (!d_super) {  // counted only: ec_graph_chains_copy compacts them
        s->hold = ec_session::Pending{2, M, ntiles, planned};
        return EC_OK;
    }
    return part_chains_copy(s, M, ntiles, planned, d_super);
}

int part_rank(ec_session *s, const SuperRec *d_all, uint64_t M) {
    hipStream_t st = s->stream;
    s->hold.kind = 0;  // (the next steps reuse the held records' buffers)
    s->chain_scr = nullptr;
    s->runs_ready = false;
    s->part_stage = 1;  // (2 once the ranking is done)
    Scalars *dsc = s->scal.as<Scalars>();
    const unsigned int N = 2 * (unsigned int)s->n_dense;
    s->stats.n_rulers = 0;
    if (!M) {
        s->part_stage = 2;
        return EC_OK;
    }
    // the super list's buffers sized by its chain count (1/16 spare on first allocation, so a
    // step whose count is a little above the last one's reuses them), not by the node count:
    // config 5's one-rank step ranks 21 M chains of 400 M nodes, where node-sized ruler state
    // held ~38 GB (r06_h)
    const size_t mc = (size_t)M + 4096;
    EC_CHECK(s->rt_srec.ensure(mc * sizeof(SuperRec), 16));
    EC_HIP(hipMemcpyAsync(s->rt_srec.p, d_all, (size_t)M * sizeof(SuperRec), hipMemcpyDeviceToDevice, st));
    k_super_index<<<grid_for(M, 256), 256, 0, st>>>(s->rt_srec.as<SuperRec>(), (unsigned int)M,
                                                    s->rt_sidx.as<unsigned int>());
    unsigned int nr = 0;
    int rounds = 0;
    if (kn().rank_sync != 1) {
        // rank_supers_async (one read-back at the end instead of one per ruler pass plus the
        // launch backlog after it): M on the device, the ruler state initialised here
        EC_CHECK(s->rt_hasp.ensure(mc, 16));
        EC_CHECK(s->rid.ensure(mc * 8, 16));
        EC_CHECK(s->st0.ensure(mc * sizeof(RJump), 16));
        EC_CHECK(s->st1.ensure(mc * sizeof(RJump), 16));
        EC_CHECK(s->rt_tbase.ensure(8));
        // the chain count on the device, the ruler state initialised: one launch (six memsets
        // cost ~40 us of launch gaps)
        k_part_rank_init<<<std::min(grid_for(M, 256), 2048u), 256, 0, st>>>(
            s->rt_tbase.as<unsigned long long>(), (unsigned int)M, s->rt_hasp.as<uint8_t>(), s->rid.as<uint2>(), &dsc->nr,
            &dsc->nvisited);
        EC_CHECK(rank_supers_async(s, N, s->rt_tbase.as<unsigned long long>(), rounds, (unsigned int)M));
        Scalars hsc{};
        EC_CHECK(d2h(s, &hsc, dsc, sizeof(Scalars), st));
        EC_CHECK(host_sync(s, st));
        note_rounds(s, hsc, rounds);
        if (hsc.nvisited == M && hsc.active[rounds - 1] == 0) {
            s->stats.n_rulers = hsc.nr;
            s->stats.rank_rounds = rounds_used(hsc, rounds);
            s->part_stage = 2;
            return EC_OK;
        }
        if (kn().verbose)
            fprintf(stderr, "part_rank: one ruler pass covered %llu of %llu chains, ranking again\n",
                    (unsigned long long)hsc.nvisited, (unsigned long long)M);
    }
    EC_CHECK(rank_supers(s, (unsigned int)M, N, nr, rounds));
    s->stats.n_rulers = nr;
    unsigned int act = 0;
    EC_CHECK(d2h(s, &act, &dsc->active[rounds - 1], 4, st));
    EC_CHECK(host_sync(s, st));
    if (act) {
        set_error("chain list ranking did not converge in %d rounds", rounds);
        return EC_ERR_STATE;
    }
    s->stats.rank_rounds = rounds;
    s->part_stage = 2;
    return EC_OK;
}

// the start records of the nodes k_starts_write listed (cnt of them) into d_starts
int part_starts_copy(ec_session *s, uint64_t cnt, StartRec *d_starts) {
    hipStream_t st = s->stream;
    if (cnt)
        k_start_recs<<<grid_for(cnt, 256), 256, 0, st>>>(s->svals.as<unsigned int>(), (unsigned int)cnt,
                                                         s->upal.as<uint8_t>(), s->dfc.as<unsigned long long>(),
                                                         s->dft.as<unsigned long long>(),
                                                         path_of(s->PK.as<unsigned int>(), s->RK.as<unsigned int>()),
                                                         s->PL.as<unsigned int>(), s->k, d_starts);
    EC_CHECK(host_sync(s, st));
    return EC_OK;
}

int part_starts(ec_session *s, bool have_supers, StartRec *d_starts, uint64_t *n_starts) {
    hipStream_t st = s->stream;
    const unsigned B = 256;
    const unsigned int n0 = (unsigned int)s->seg_n0, n1 = (unsigned int)s->seg_n1;
    const size_t Nn = std::max<size_t>(2 * (size_t)s->n_dense, 1);
    *n_starts = 0;
    s->hold.kind = 0;
    s->runs_ready = false;
    s->part_stage = 2;  // (3 once the starts are listed)
    if (n1 <= n0) {  // an empty segment (a rank that owns no solid key): no starts, counted as such
        s->part_stage = 3;
        if (!d_starts) s->hold = ec_session::Pending{3, 0, 0, false};
        return EC_OK;
    }
    if (have_supers)
        k_expand<<<grid_for(n1 - n0, B), B, 0, st>>>(s->pred.as<unsigned int>(), s->rt_lr.as<unsigned int>(), n1,
                                                     s->rt_sidx.as<unsigned int>(), s->rt_pks.as<unsigned int>(),
                                                     s->rt_rks.as<unsigned int>(), s->PK.as<unsigned int>(),
                                                     s->RK.as<unsigned int>(), n0);
    const unsigned int nblk = (n1 - n0 + RULER_CHUNK - 1) / RULER_CHUNK;
    EC_CHECK(s->rbc.ensure((size_t)nblk * 8 + 8));
    EC_CHECK(s->cand.ensure(((size_t)(n1 - n0) / 64 + 8) * 8));
    EC_CHECK(s->skeys.ensure(Nn * 8));
    EC_CHECK(s->svals.ensure(Nn * 4));
    unsigned int *bc = s->rbc.as<unsigned int>(), *bs = bc + nblk;
    k_starts_count<<<nblk, B, 0, st>>>(s->upal.as<uint8_t>(), s->dfc.as<unsigned long long>(),
                                       s->dft.as<unsigned long long>(), path_of(s->PK.as<unsigned int>(), s->RK.as<unsigned int>()),
                                       s->PM.as<unsigned long long>(), n1, bc, s->cand.as<unsigned long long>(), nullptr,
                                       n0);
    EC_CHECK(scan_incl_u32(s, bc, bs, nblk));
    k_starts_write<<<nblk, B, 0, st>>>(s->upal.as<uint8_t>(), s->dfc.as<unsigned long long>(),
                                       s->dft.as<unsigned long long>(), path_of(s->PK.as<unsigned int>(), s->RK.as<unsigned int>()),
                                       s->PM.as<unsigned long long>(), n1, bs, s->cand.as<unsigned long long>(),
                                       s->skeys.as<unsigned long long>(), s->svals.as<unsigned int>(), n0);
    unsigned int cnt = 0;
    EC_CHECK(d2h(s, &cnt, bs + nblk - 1, 4, st));
    EC_CHECK(host_sync(s, st));
    *n_starts = cnt;
    s->part_stage = 3;
    if (!d_starts) {  // counted only: ec_graph_starts_copy writes them
        s->hold = ec_session::Pending{3, cnt, 0, false};
        return EC_OK;
    }
    return part_starts_copy(s, cnt, d_starts);
}

int part_layout(ec_session *s, const StartRec *d_all, uint64_t nc, uint64_t *n_chars) {
    hipStream_t st = s->stream;
    s->hold.kind = 0;
    s->runs_ready = false;  // (runs emitted under an earlier layout: their chunk counts do not fit this one)
    s->part_stage = 3;      // (4 once the layout stands)
    const unsigned B = 256;
    const size_t Nn = std::max<size_t>(2 * (size_t)s->n_dense, 1), nn = std::max<size_t>(nc, 1);
    EC_CHECK(s->skeys.ensure(nn * 8));
    EC_CHECK(s->svals.ensure(nn * 4));
    EC_CHECK(s->skeys2.ensure(nn * 8));
    EC_CHECK(s->svals2.ensure(nn * 4));
    EC_CHECK(s->clen.ensure((nn + 1) * 8));
    EC_CHECK(s->coff.ensure((nn + 1) * 8));
    EC_CHECK(s->cwalk.ensure(nn * sizeof(Walk)));
    EC_CHECK(s->cidxOf.ensure(Nn * 4));
    EC_HIP(hipMemsetAsync(s->cidxOf.p, 0xFF, Nn * 4, st));
    EC_HIP(hipMemsetAsync(s->clen.as<unsigned long long>() + nc, 0, 8, st));
    if (nc) {
        k_start_keys<<<grid_for(nc, B), B, 0, st>>>(d_all, (unsigned int)nc, s->skeys.as<unsigned long long>(),
                                                    s->svals.as<unsigned int>());
        EC_CHECK(sort_pairs(s, s->skeys.as<unsigned long long>(), s->skeys2.as<unsigned long long>(),
                            s->svals.as<unsigned int>(), s->svals2.as<unsigned int>(), nc));
        k_layout<<<grid_for(nc, B), B, 0, st>>>(d_all, s->svals2.as<unsigned int>(), (unsigned int)nc,
                                                s->clen.as<unsigned long long>(), s->cidxOf.as<unsigned int>(),
                                                s->cwalk.as<Walk>());
    }
    EC_CHECK(scan_u64(s, s->clen.as<unsigned long long>(), s->coff.as<unsigned long long>(), nc + 1));
    unsigned long long tot = 0;
    EC_CHECK(d2h(s, &tot, s->coff.as<unsigned long long>() + nc, 8, st));
    EC_CHECK(host_sync(s, st));
    s->seg_nc = (unsigned int)nc;
    s->seg_nchars = tot;
    *n_chars = tot;
    s->part_stage = 4;
    return EC_OK;
}

template <typename Ops>
int part_emit(ec_session *s, char *d_chars, void *d_ends, bool check = true) {
    hipStream_t st = s->stream;
    const unsigned B = 256;
    Scalars *dsc = s->scal.as<Scalars>();
    const unsigned int n0 = (unsigned int)s->seg_n0, n1 = (unsigned int)s->seg_n1, nc = s->seg_nc;
    const size_t Nn = std::max<size_t>(2 * (size_t)s->n_dense, 1), nn = std::max<size_t>(nc, 1);
    EC_CHECK(s->cfirst.ensure(nn * 4));
    EC_CHECK(s->clast.ensure(nn * 4));
    EC_CHECK(s->headOf.ensure(Nn * 4));
    EC_CHECK(s->tailOf.ensure(Nn * 4));
    EC_HIP(hipMemsetAsync(s->cfirst.p, 0xFF, nn * 4, st));
    EC_HIP(hipMemsetAsync(s->clast.p, 0xFF, nn * 4, st));
    EC_HIP(hipMemsetAsync(&dsc->skew, 0, 4, st));
    EC_CHECK(s->ewalk.ensure(nn * sizeof(EWalk)));
    if (nc)
        k_ewalk<<<grid_for(nc, B), B, 0, st>>>(s->cwalk.as<Walk>(), s->coff.as<unsigned long long>(), nc,
                                              s->ewalk.as<EWalk>());
    if (n1 > n0 && nc)
        k_emit<Ops><<<grid_for(n1 - n0, B), B, 0, st>>>(
            s->upal.as<uint8_t>(), path_of(s->PK.as<unsigned int>(), s->RK.as<unsigned int>()),
            s->PL.as<unsigned int>(), s->dkey.as<typename Ops::K>(), s->cidxOf.as<unsigned int>(), s->ewalk.as<EWalk>(),
            n1, s->k, d_chars, std::max<uint64_t>(s->seg_nchars, 1),
            s->cfirst.as<unsigned int>(), s->clast.as<unsigned int>(), s->headOf.as<unsigned int>(),
            s->tailOf.as<unsigned int>(), &dsc->skew, n0);
    // contig ends as k-mer codes (the collecting rank holds no global set): 2 nc codes, each
    // written by the rank that emitted the node, zeros elsewhere
    if (nc && d_ends)
        k_ends_codes<Ops><<<grid_for(nc, B), B, 0, st>>>(s->cfirst.as<unsigned int>(), s->clast.as<unsigned int>(), nc,
                                                         s->dkey.as<typename Ops::K>(), s->k,
                                                         reinterpret_cast<typename Ops::K *>(d_ends));
    if (!check) return EC_OK;  // (the caller reads dsc->skew with its own scalars)
    unsigned int bad = 0;
    EC_CHECK(d2h(s, &bad, &dsc->skew, 4, st));
    EC_CHECK(host_sync(s, st));
    if (bad) {
        set_error("contig characters past their bound %llu (inconsistent ranking)", (unsigned long long)s->seg_nchars);
        return EC_ERR_STATE;
    }
    s->part_stage = 5;
    return EC_OK;
}

template <typename Ops>
int part_collect(ec_session *s, const char *d_chars, const void *d_ends_v, uint64_t n_pal, bool packable = false) {
    using K = typename Ops::K;
    using T = typename EndSlotOf<K>::T;
    hipStream_t st = s->stream;
    const unsigned B = 256;
    const unsigned int U = (unsigned int)s->n_dense, nc = s->seg_nc;
    const size_t nn = std::max<size_t>(nc, 1);
    const uint64_t nchars = s->seg_nchars;
    const K *d_ends = static_cast<const K *>(d_ends_v);
    EC_CHECK(s->lk.ensure(nn * 16 * 8));
    EC_CHECK(s->lcnt.ensure(nn * 2 * 4));
    if (nc) {  // GFA links from the contig-end codes (junction.h): a table of 2 nc entries
        uint64_t cap = 1024;
        while (cap < 4ull * nc) cap <<= 1;
        EC_CHECK(s->table.ensure(cap * sizeof(T)));
        T *t = s->table.as<T>();
        if (sizeof(K) == 8) k_end_clear64<<<grid_for(cap, B, 8192), B, 0, st>>>(reinterpret_cast<EndSlot64 *>(t), cap);
        else k_end_clearW<<<grid_for(cap, B, 8192), B, 0, st>>>(reinterpret_cast<EndSlotW *>(t), cap);
        k_end_insert<Ops><<<grid_for(nc, B), B, 0, st>>>(d_ends, nc, s->k, t, cap - 1);
        k_gfa_codes<Ops><<<grid_for(nc, B), B, 0, st>>>(d_ends, nc, s->k, t, cap - 1, s->lk.as<long long>(),
                                                        s->lcnt.as<unsigned int>());
    }
    const unsigned int n2 = 2 * nc;
    s->links_compact = false;
    EC_CHECK(s->h_coff.resize((size_t)nc + 1));
    EC_CHECK(s->h_loff.resize((size_t)n2 + 1));
    s->h_loff[n2] = 0;
    EC_CHECK(d2h(s, s->h_coff.data(), s->coff.p, ((size_t)nc + 1) * 8, st));
    if (nc) {
        EC_CHECK(s->skeys.ensure(((size_t)n2 + 1) * 8));
        EC_CHECK(s->skeys2.ensure(((size_t)n2 + 1) * 8));
        k_lcnt64<<<grid_for(n2 + 1ull, B), B, 0, st>>>(s->lcnt.as<unsigned int>(), n2, s->skeys.as<unsigned long long>());
        EC_CHECK(scan_u64(s, s->skeys.as<unsigned long long>(), s->skeys2.as<unsigned long long>(), (size_t)n2 + 1));
        EC_CHECK(d2h(s, s->h_loff.data(), s->skeys2.p, ((size_t)n2 + 1) * 8, st));
    }
    // (d_chars of the session, 16 B padded: the characters travel as 2-bit codes, as phase_graph's)
    const bool pack = packable && !std::is_same<Ops, OpsX>::value && kn().no_char_pack == 0;
    s->chars_packed = pack;
    s->nchars_host = nchars;
    if (pack) {
        const uint64_t cap16 = (nchars + 15) / 16;
        EC_CHECK(s->dchars.ensure(std::max<uint64_t>(cap16, 1) * 4));
        if (cap16)
            k_pack_chars<<<std::min(grid_for(cap16, B), 8192u), B, 0, st>>>(
                reinterpret_cast<const uint4 *>(d_chars), s->coff.as<unsigned long long>() + nc, cap16,
                s->dchars.as<uint32_t>());
        EC_CHECK(s->h_chars.resize((nchars + 3) / 4));
        if (nchars) EC_CHECK(d2h(s, s->h_chars.data(), s->dchars.p, (nchars + 3) / 4, st));
    } else {
        EC_CHECK(s->h_chars.resize(nchars));
        if (nchars) EC_CHECK(d2h(s, s->h_chars.data(), d_chars, nchars, st));
    }
    EC_CHECK(host_sync(s, st));
    const uint64_t nlinks = s->h_loff[n2];
    EC_CHECK(s->h_links.resize(nlinks));
    if (nlinks) {
        EC_CHECK(s->dcounts.ensure(nlinks * 8));
        k_links_compact<long long><<<grid_for(n2, B), B, 0, st>>>(s->lk.as<long long>(), s->lcnt.as<unsigned int>(),
                                                                 s->skeys2.as<unsigned long long>(), n2,
                                                                 s->dcounts.as<long long>());
        EC_CHECK(d2h(s, s->h_links.data(), s->dcounts.p, nlinks * 8, st));
    }
    EC_CHECK(host_sync(s, st));
    s->stats.n_solid = U;
    s->stats.n_contigs = nc;
    s->stats.n_contig_chars = nchars;
    s->stats.n_links = nlinks;
    s->stats.n_dict = 2ull * U - n_pal;
    s->have = true;
    s->stats_ok = true;
    return EC_OK;
}

// ---- the partitioned finish's transfer to the collecting rank (junction.h, round 6) -----------
// this rank's emission into a zeroed job-sized buffer of its own (never sent), its runs counted
// per chunk and scanned, its contig ends as records; one read-back for the sizes
template <typename Ops>
int part_emit_runs(ec_session *s, uint64_t *nbytes) {
    using K = typename Ops::K;
    hipStream_t st = s->stream;
    const unsigned B = 256;
    Scalars *dsc = s->scal.as<Scalars>();
    const uint64_t nchars = s->seg_nchars;
    const unsigned int nc = s->seg_nc;
    s->runs_ready = false;
    EC_CHECK(s->chars.ensure(nchars + 32));
    EC_HIP(hipMemsetAsync(s->chars.p, 0, nchars + 32, st));
    EC_CHECK(part_emit<Ops>(s, s->chars.as<char>(), nullptr, false));
    const uint64_t nch = (nchars + RUN_CH - 1) / RUN_CH;
    EC_CHECK(s->run_cnt.ensure(4 * (nch + 1) * 8));
    unsigned long long *rc = s->run_cnt.as<unsigned long long>(), *cc = rc + nch + 1, *rb = cc + nch + 1,
                       *cb = rb + nch + 1;
    EC_HIP(hipMemsetAsync(rc, 0, 2 * (nch + 1) * 8, st));
    if (nch) k_runs_count<<<(unsigned)nch, RUN_NT, 0, st>>>(s->chars.as<uint8_t>(), nchars, rc, cc);
    EC_CHECK(scan_u64(s, rc, rb, nch + 1));
    EC_CHECK(scan_u64(s, cc, cb, nch + 1));
    EC_CHECK(s->run_ends.ensure(std::max<size_t>(2ull * nc, 1) * sizeof(EndRec<K>)));
    EC_CHECK(s->jcnt.ensure(16));
    unsigned int *nout = s->jcnt.as<unsigned int>();
    EC_HIP(hipMemsetAsync(nout, 0, 4, st));
    if (nc)
        k_ends_recs<Ops><<<grid_for(nc, B), B, 0, st>>>(s->cfirst.as<unsigned int>(), s->clast.as<unsigned int>(), nc,
                                                        s->dkey.as<K>(), s->k, s->run_ends.as<EndRec<K>>(), nout);
    unsigned long long tot[2] = {0, 0};
    unsigned int ne = 0, bad = 0;
    EC_CHECK(d2h(s, &tot[0], rb + nch, 8, st));
    EC_CHECK(d2h(s, &tot[1], cb + nch, 8, st));
    EC_CHECK(d2h(s, &ne, nout, 4, st));
    EC_CHECK(d2h(s, &bad, &dsc->skew, 4, st));
    EC_CHECK(host_sync(s, st));
    if (bad) {
        set_error("contig characters past their bound %llu (inconsistent ranking)", (unsigned long long)nchars);
        return EC_ERR_STATE;
    }
    s->run_nr = tot[0];
    s->run_nch = tot[1];
    s->run_nends = ne;
    s->runs_ready = true;
    s->part_stage = 5;
    *nbytes = run_rec_bytes(tot[0], tot[1], ne, (int)sizeof(K));
    return EC_OK;
}

// the transfer record into d_out (ec_graph_emit_runs' size), stream-ordered (no sync)
template <typename Ops>
int part_copy_runs(ec_session *s, void *d_out) {
    using K = typename Ops::K;
    hipStream_t st = s->stream;
    const uint64_t nchars = s->seg_nchars, nch = (nchars + RUN_CH - 1) / RUN_CH, nr = s->run_nr;
    unsigned long long *rc = s->run_cnt.as<unsigned long long>(), *rb = rc + 2 * (nch + 1), *cb = rb + nch + 1;
    unsigned long long *hdr = static_cast<unsigned long long *>(d_out);
    unsigned long long *rstart = hdr + 4, *rcoff = rstart + nr;
    uint8_t *rchars = reinterpret_cast<uint8_t *>(rcoff + nr);
    uint8_t *ends = rchars + ((s->run_nch + 7) & ~7ull);
    k_put_u64x4<<<1, 64, 0, st>>>(hdr, nr, s->run_nch, s->run_nends, 0ull);
    if (nch) k_runs_write<<<(unsigned)nch, RUN_NT, 0, st>>>(s->chars.as<uint8_t>(), nchars, rb, cb, rstart, rcoff, rchars);
    if (s->run_nends)
        EC_HIP(hipMemcpyAsync(ends, s->run_ends.p, s->run_nends * sizeof(EndRec<K>), hipMemcpyDeviceToDevice, st));
    return EC_OK;
}

// the collecting rank: every rank's transfer record (concatenated, src_bytes each) into the
// job's characters and end table, then part_collect
template <typename Ops>
int part_collect_runs(ec_session *s, const uint8_t *d_in, int nsrc, const uint64_t *src_bytes, uint64_t n_pal) {
    using K = typename Ops::K;
    hipStream_t st = s->stream;
    const unsigned B = 256;
    const uint64_t nchars = s->seg_nchars;
    const unsigned int nc = s->seg_nc;
    std::vector<unsigned long long> hdr(4 * (size_t)nsrc);
    uint64_t o = 0;
    for (int r = 0; r < nsrc; r++) {
        if (src_bytes[r] < 32 || (o & 7)) {
            set_error("ec_graph_collect_runs: source %d's record is %llu bytes at offset %llu", r,
                      (unsigned long long)src_bytes[r], (unsigned long long)o);
            return EC_ERR_ARG;
        }
        EC_CHECK(d2h(s, &hdr[4 * r], d_in + o, 32, st));
        o += src_bytes[r];
    }
    EC_CHECK(host_sync(s, st));
    s->runs_ready = false;  // (the job's characters go where this rank's emitted runs were)
    EC_CHECK(s->chars.ensure(nchars + 32));
    EC_CHECK(s->run_dends.ensure(std::max<size_t>(2ull * nc, 1) * sizeof(K)));
    EC_HIP(hipMemsetAsync(s->run_dends.p, 0, std::max<size_t>(2ull * nc, 1) * sizeof(K), st));
    EC_CHECK(s->jcnt.ensure(16));
    unsigned int *bad = s->jcnt.as<unsigned int>();
    EC_HIP(hipMemsetAsync(bad, 0, 4, st));
    o = 0;
    for (int r = 0; r < nsrc; r++) {
        const uint64_t nr = hdr[4 * r], nch = hdr[4 * r + 1], ne = hdr[4 * r + 2];
        if (run_rec_bytes(nr, nch, ne, (int)sizeof(K)) != src_bytes[r]) {
            set_error("ec_graph_collect_runs: source %d's record holds %llu bytes, its header %llu", r,
                      (unsigned long long)src_bytes[r], (unsigned long long)run_rec_bytes(nr, nch, ne, (int)sizeof(K)));
            return EC_ERR_ARG;
        }
        const unsigned long long *rstart = reinterpret_cast<const unsigned long long *>(d_in + o) + 4;
        const unsigned long long *rcoff = rstart + nr;
        const uint8_t *rchars = reinterpret_cast<const uint8_t *>(rcoff + nr);
        const EndRec<K> *ends = reinterpret_cast<const EndRec<K> *>(rchars + ((nch + 7) & ~7ull));
        if (nr)
            k_runs_scatter<<<std::min(grid_for(nr, B), 8192u), B, 0, st>>>(rstart, rcoff, nr, nch, rchars,
                                                                         s->chars.as<uint8_t>(), nchars, bad);
        if (ne)
            k_ends_scatter<K><<<grid_for(ne, B), B, 0, st>>>(ends, ne, 2 * nc, s->run_dends.as<K>(), bad);
        o += src_bytes[r];
    }
    unsigned int hb = 0;
    EC_CHECK(d2h(s, &hb, bad, 4, st));
    EC_CHECK(host_sync(s, st));
    if (hb) {
        set_error("ec_graph_collect_runs: a run or an end outside the layout");
        return EC_ERR_ARG;
    }
    return part_collect<Ops>(s, s->chars.as<char>(), s->run_dends.p, n_pal, true);
}

// ---- extended alphabet (extended.h) -----------------------------------------------------------
// c_xa (the symbol table the OpsX kernels read) is one per process: extended-alphabet calls
// of different sessions are serialised (each call ends with its stream synchronised)
std::mutex g_xmu;

int x_upload(ec_session *s) {
    EC_HIP(hipMemcpyToSymbolAsync(HIP_SYMBOL(c_xa), &s->xa, sizeof(XAlpha), 0, hipMemcpyHostToDevice, s->stream));
    return EC_OK;
}

// the symbol table from the bytes present (bit c of pm): A C G T = 0..3, 'N' the segment split
// (split_n) or an opaque symbol, every other byte an opaque symbol in byte order
int x_alphabet(ec_session *s, const unsigned int *pm, bool split_n, int k) {
    XAlpha &xa = s->xa;
    memset(&xa, 0, sizeof xa);
    const char *acgt = "ACGT";
    for (int c = 0; c < 256; c++) xa.code[c] = 0xFE;
    for (int b = 0; b < 4; b++) xa.code[(int)acgt[b]] = (uint8_t)b, xa.dec[b] = (uint8_t)acgt[b];
    if (split_n) xa.code[(int)'N'] = 0xFF;
    unsigned int nsym = 4;
    for (int c = 0; c < 256; c++)
        if (((pm[c >> 5] >> (c & 31)) & 1u) && xa.code[c] == 0xFE) {
            xa.code[c] = (uint8_t)nsym;
            xa.dec[nsym++] = (uint8_t)c;
        }
    xa.nsym = nsym;
    xa.sb = nsym <= 16 ? 4 : nsym <= 32 ? 5 : 8;
    if (xa.sb * (unsigned)k > 126) {
        set_error("the input holds %u symbols besides A/C/G/T%s (%u bits each): k = %d needs %u-bit keys, more than "
                  "126 (k <= %u for this alphabet)", nsym - 4, split_n ? "/N" : "", xa.sb, k, xa.sb * k, 126 / xa.sb);
        return EC_ERR_ALPHABET;
    }
    EC_CHECK(x_upload(s));
    s->xalpha = true;
    return EC_OK;
}

// all_contigs on a caller's dict holding bytes other than A/C/G/T (ec_assemble_from_kmers)
int assemble_kmers_extended(ec_session *s, const char *kmers, uint64_t n, int k) {
    std::lock_guard<std::mutex> lock(g_xmu);
    unsigned int pm[8] = {};
    for (uint64_t i = 0; i < n * (uint64_t)k; i++) {
        const unsigned char c = (unsigned char)kmers[i];
        pm[c >> 5] |= 1u << (c & 31);
    }
    EC_CHECK(x_alphabet(s, pm, false, k));
    hipStream_t st = s->stream;
    k_x_kmers_to_agg<<<grid_for(n, 256), 256, 0, st>>>(s->dchars.as<char>(), s->dcounts.as<unsigned int>(), n, k,
                                                       s->recs2.as<AggW>());
    unsigned int U = 0;
    SolidIndexW sidx{};
    EC_CHECK(phase_merge_w(s, s->recs2.as<AggW>(), n, LLONG_MIN, U, sidx));
    return phase_graph<OpsX>(s, k, U, sidx);
}

// reads with bytes other than A/C/G/T/N: symbol table from the bytes present, count into the
// wide HBM table (128-bit keys of sb-bit symbols), then the graph phase over OpsX
int assemble_extended(ec_session *s, const uint8_t *d_reads, const uint64_t *d_off, uint64_t nreads, int k,
                      long long limit) {
    std::lock_guard<std::mutex> lock(g_xmu);
    hipStream_t st = s->stream;
    const unsigned B = 256;
    Scalars *dsc = s->scal.as<Scalars>();
    Scalars hsc;
    EC_CHECK(s->tmp.ensure(64));
    unsigned int *present = s->tmp.as<unsigned int>();
    EC_HIP(hipMemsetAsync(present, 0, 32, st));
    if (nreads) k_x_alphabet<<<grid_for(nreads, B, 4096), B, 0, st>>>(d_reads, d_off, nreads, present);
    unsigned int pm[8];
    EC_CHECK(d2h(s, pm, present, 32, st));
    EC_CHECK(host_sync(s, st));
    EC_CHECK(x_alphabet(s, pm, true, k));
    s->stats.count_variant = 0;
    s->stats.n_buckets = 0;
    s->stats.record_bytes = 0;
    s->stats.n_records = 0;
    s->stats.n_reads = nreads;
    // prescan (positions, HyperLogLog of the canonical keys) + count (phase_count_w's table)
    mark(s, 2 * EC_STAGE_PRESCAN);
    EC_CHECK(s->hll.ensure(HLL_M * 4));
    EC_HIP(hipMemsetAsync(s->hll.p, 0, HLL_M * 4, st));
    EC_HIP(hipMemsetAsync(&dsc->npos, 0, 8, st));
    EC_HIP(hipMemsetAsync(&dsc->est, 0, 8, st));
    if (nreads) {
        k_x_prescan<<<grid_for(nreads, B, 4096), B, 0, st>>>(d_reads, d_off, nreads, k, s->hll.as<unsigned int>(),
                                                            &dsc->npos);
        k_hll_final<<<1, 1024, 0, st>>>(s->hll.as<unsigned int>(), HLL_BITS, &dsc->est);
    }
    mark(s, 2 * EC_STAGE_PRESCAN + 1);
    EC_CHECK(d2h(s, &hsc, dsc, sizeof(Scalars), st));
    EC_CHECK(host_sync(s, st));
    const uint64_t P = nreads ? hsc.npos : 0;
    s->stats.n_positions = P;
    const double est = nreads ? hsc.est : 0.0;
    s->stats.n_distinct_est = (uint64_t)llround(est);
    uint64_t cap = 1024;
    const double want = std::min((double)P, 1.05 * est) * 1.6 + 1024;
    while ((double)cap < want) cap <<= 1;
    for (int attempt = 0;; attempt++) {
        EC_CHECK(s->table.ensure(cap * sizeof(SlotW)));
        mark(s, 2 * EC_STAGE_COUNT);
        k_table_clear_w<<<grid_for(cap, B, 8192), B, 0, st>>>(s->table.as<SlotW>(), cap);
        EC_HIP(hipMemsetAsync(&dsc->overflow, 0, 4, st));
        if (nreads) {
            kmark(s, 3, 0);
            k_x_count<<<grid_for(nreads, B), B, 0, st>>>(d_reads, d_off, nreads, k, s->table.as<SlotW>(), cap - 1,
                                                        &dsc->overflow);
            kmark(s, 3, 1);
        }
        mark(s, 2 * EC_STAGE_COUNT + 1);
        EC_CHECK(d2h(s, &hsc.overflow, &dsc->overflow, 4, st));
        EC_CHECK(host_sync(s, st));
        if (!hsc.overflow) break;
        if (attempt >= 4) {
            set_error("hash table overflow at capacity %llu", (unsigned long long)cap);
            return EC_ERR_CAPACITY;
        }
        cap <<= 2;
        s->stats.table_retries++;
    }
    unsigned int U = 0;
    SolidIndexW sidx{};
    EC_CHECK(finish_wide(s, cap, limit, U, sidx));
    return phase_graph<OpsX>(s, k, U, sidx);
}

int assemble(ec_session *s, const uint8_t *d_reads, const uint64_t *d_off, uint64_t nreads, int k, int limit,
             unsigned flags) {
    EC_CHECK(begin_call(s, k, flags));
    unsigned int U = 0;
    if (k > 32) {
        SolidIndexW sidx{};
        EC_CHECK(pipe_all(s));
        const int rc = phase_count_w(s, d_reads, d_off, nreads, 0, k, (long long)limit, U, sidx);
        if (rc == EC_ERR_ALPHABET) return assemble_extended(s, d_reads, d_off, nreads, k, (long long)limit);
        EC_CHECK(rc);
        return phase_graph<OpsW>(s, k, U, sidx);
    }
    SolidIndex sidx{};
    s->graph_follows = true;  // (phase_graph<Ops64> below: phase_count_sk2 may queue links_local's prologue)
    const int rc = phase_count(s, d_reads, d_off, nreads, 0, k, (long long)limit, flags, U, sidx);
    if (rc == EC_ERR_ALPHABET) {  // bytes other than A/C/G/T/N: opaque symbols (extended.h)
        EC_CHECK(pipe_all(s));
        return assemble_extended(s, d_reads, d_off, nreads, k, (long long)limit);
    }
    EC_CHECK(rc);
    return phase_graph<Ops64>(s, k, U, sidx);
}

// ---- host input -------------------------------------------------------------------------------
using Pipe = ec_session::Pipe;
// Chunk plan over nbases bases (chunk boundaries at multiples of 64 bases, ~32 MiB of copied
// bytes a chunk) and the reads each chunk completes (offsets: host array, or NULL = one length L)
int pipe_plan(ec_session *s, Pipe &pp, uint64_t nbases, uint64_t bytes_per_base4, const uint64_t *offsets,
              uint64_t nreads, uint64_t L, hipEvent_t after = nullptr) {
    const uint64_t copy_bytes = bytes_per_base4 ? (nbases + 3) / 4 : nbases;
    int nc = (int)std::min<uint64_t>(64, std::max<uint64_t>(1, copy_bytes >> 25));
    if (kn().host_chunks) nc = std::max(1, std::min(64, kn().host_chunks));
    pp.nchunks = nc;
    pp.done = 0;
    pp.blo.assign(nc, 0), pp.bhi.assign(nc, 0), pp.ravail.assign(nc, 0), pp.elo.assign(nc, 0), pp.ehi.assign(nc, 0);
    for (int c = 0; c < nc; c++) {
        pp.blo[c] = c ? pp.bhi[c - 1] : 0;
        pp.bhi[c] = c + 1 == nc ? nbases : std::max<uint64_t>(pp.blo[c], (nbases * (uint64_t)(c + 1) / nc) & ~63ull);
        uint64_t r;  // reads with offsets[r + 1] <= bhi
        if (c + 1 == nc) r = nreads;
        else if (!offsets) r = L ? std::min<uint64_t>(nreads, pp.bhi[c] / L) : nreads;
        else r = (uint64_t)(std::upper_bound(offsets + 1, offsets + nreads + 1, pp.bhi[c]) - (offsets + 1));
        pp.ravail[c] = r;
    }
    if ((int)pp.ev.size() < nc) {
        const size_t have = pp.ev.size();
        pp.ev.resize(nc, nullptr);
        for (size_t i = have; i < (size_t)nc; i++) EC_HIP(hipEventCreateWithFlags(&pp.ev[i], hipEventDisableTiming));
    }
    if (!s->cstream) EC_HIP(hipStreamCreateWithFlags(&s->cstream, hipStreamNonBlocking));
    // the copies overwrite buffers a previous call's kernels may still read: after = the event
    // of their last reader (a staged slot), else everything queued on the session stream
    if (!after) {
        EC_HIP(hipEventRecord(pp.ev[0], s->stream));
        after = pp.ev[0];
    }
    EC_HIP(hipStreamWaitEvent(s->cstream, after, 0));
    return EC_OK;
}

// copy the offsets entries reads [r0, r1] need (chunk by chunk: [ravail[c-1] + 1, ravail[c] + 1))
int pipe_copy_offsets(ec_session *s, const Pipe &pp, int c, const uint64_t *offsets, uint64_t *d_off) {
    const uint64_t o0 = c ? pp.ravail[c - 1] + 1 : 0, o1 = pp.ravail[c] + 1;
    if (o1 > o0)
        EC_HIP(hipMemcpyAsync(d_off + o0, offsets + o0, (o1 - o0) * 8, hipMemcpyHostToDevice, s->cstream));
    return EC_OK;
}

int check_offsets(const uint64_t *offsets, uint64_t nreads, uint64_t nbytes) {
    if (offsets[nreads] > nbytes) {
        set_error("offsets[nreads]=%llu > nbytes=%llu", (unsigned long long)offsets[nreads], (unsigned long long)nbytes);
        return EC_ERR_ARG;
    }
    for (uint64_t i = 0; i < nreads; i++)
        if (offsets[i] > offsets[i + 1]) {
            set_error("offsets not monotone at %llu", (unsigned long long)i);
            return EC_ERR_ARG;
        }
    return EC_OK;
}

// run assemble() on the pipelined input; the pipeline is drained (every chunk consumed) on any
// return so no chunk copy is left pending against the next call's buffers
int assemble_piped(ec_session *s, const uint64_t *d_off, uint64_t nreads, int k, int limit, unsigned flags) {
    s->pipe.active = true;
    s->pipe.ascii = s->h_reads.as<uint8_t>();  // (staged batches: h_reads may have grown since)
    int rc = EC_OK;
    // copies already complete (a staged batch, copied while the previous one assembled): the
    // count runs once over the whole batch -- per-chunk partition launches fill the chip only
    // a seventh at a time (7 x 0.34 ms against 0.98 ms for one launch at the headline)
    if (s->pipe.nchunks > 1 && s->pipe.done < s->pipe.nchunks &&
        hipEventQuery(s->pipe.ev[s->pipe.nchunks - 1]) == hipSuccess)
        rc = pipe_all(s);
    if (rc == EC_OK) rc = assemble(s, s->h_reads.as<uint8_t>(), d_off, nreads, k, limit, flags);
    if (s->pipe.done < s->pipe.nchunks) {
        pipe_all(s);
        (void)host_sync(s, s->stream);
    }
    s->pipe.active = false;
    return rc;
}

int check_packed(const uint8_t *codes, uint64_t nbases, const uint64_t *offsets, uint64_t nreads, uint32_t read_len,
                 const uint64_t *exc_pos, const uint8_t *exc_byte, uint64_t n_exc) {
    if ((nbases && !codes) || (n_exc && (!exc_pos || !exc_byte))) {
        set_error("null argument");
        return EC_ERR_ARG;
    }
    if (offsets) {
        EC_CHECK(check_offsets(offsets, nreads, nbases));
    } else if ((uint64_t)read_len * nreads != nbases) {
        set_error("%llu reads of %u bases != %llu bases", (unsigned long long)nreads, read_len,
                  (unsigned long long)nbases);
        return EC_ERR_ARG;
    }
    for (uint64_t i = 0; i < n_exc; i++)
        if (exc_pos[i] >= nbases || (i && exc_pos[i] <= exc_pos[i - 1])) {
            set_error("exception %llu: position %llu not ascending inside [0, %llu)", (unsigned long long)i,
                      (unsigned long long)exc_pos[i], (unsigned long long)nbases);
            return EC_ERR_ARG;
        }
    return EC_OK;
}

// a packed batch's copies into (codes_b, exc_b, off_b) on cstream, chunk events in pp (the
// plan of assemble_piped); after = the event the copies wait for (nullptr: the session stream)
int stage_packed(ec_session *s, Pipe &pp, DevBuf &codes_b, DevBuf &exc_b, DevBuf &off_b, hipEvent_t after,
                 const uint8_t *codes, uint64_t nbases, const uint64_t *offsets, uint64_t nreads, uint32_t read_len,
                 const uint64_t *exc_pos, const uint8_t *exc_byte, uint64_t n_exc) {
    const uint64_t ncodes = (nbases + 3) / 4;
    EC_CHECK(off_b.ensure((nreads + 1) * 8));
    EC_CHECK(codes_b.ensure(((ncodes + 3) & ~3ull) + 16));
    EC_CHECK(exc_b.ensure(n_exc * 9 + 16));
    EC_CHECK(pipe_plan(s, pp, nbases, 1, offsets, nreads, read_len, after));
    pp.packed = true;
    pp.first_len = nreads ? (offsets ? offsets[1] - offsets[0] : read_len) : 0;
    pp.codes = codes_b.as<uint32_t>();
    pp.exc_pos = exc_b.as<uint64_t>();
    pp.exc_byte = exc_b.as<uint8_t>() + n_exc * 8;
    if (n_exc) {
        EC_HIP(hipMemcpyAsync(exc_b.p, exc_pos, n_exc * 8, hipMemcpyHostToDevice, s->cstream));
        EC_HIP(hipMemcpyAsync(exc_b.as<uint8_t>() + n_exc * 8, exc_byte, n_exc, hipMemcpyHostToDevice, s->cstream));
    }
    if (!offsets)  // one read length: the offsets are made on the device (ordered before chunk 0's event)
        k_iota_off<<<grid_for(nreads + 1, 256, 16384), 256, 0, s->cstream>>>(off_b.as<uint64_t>(), nreads + 1, read_len);
    for (int c = 0; c < pp.nchunks; c++) {
        // code bytes of bases [blo, bhi) (blo a multiple of 64: whole 32-bit words)
        const uint64_t c0 = pp.blo[c] / 4, c1 = c + 1 == pp.nchunks ? ncodes : pp.bhi[c] / 4;
        if (c1 > c0)
            EC_HIP(hipMemcpyAsync(codes_b.as<uint8_t>() + c0, codes + c0, c1 - c0, hipMemcpyHostToDevice, s->cstream));
        if (offsets) EC_CHECK(pipe_copy_offsets(s, pp, c, offsets, off_b.as<uint64_t>()));
        pp.elo[c] = (uint64_t)(std::lower_bound(exc_pos, exc_pos + n_exc, pp.blo[c]) - exc_pos);
        pp.ehi[c] = (uint64_t)(std::lower_bound(exc_pos, exc_pos + n_exc, pp.bhi[c]) - exc_pos);
        EC_HIP(hipEventRecord(pp.ev[c], s->cstream));
    }
    return EC_OK;
}

}  // namespace

// 2-bit codes (4 a byte, first character in the low bits) -> n ASCII characters; threads past
// ~4 MB of characters (ecoli10m_err: 38 MB)
static void unpack_codes(const uint8_t *codes, uint64_t n, char *out) {
    static const struct Lut {
        uint32_t v[256];
        Lut() {
            const char acgt[4] = {'A', 'C', 'G', 'T'};
            for (int b = 0; b < 256; b++) {
                uint32_t w = 0;
                for (int j = 0; j < 4; j++) w |= (uint32_t)(uint8_t)acgt[(b >> (2 * j)) & 3] << (8 * j);
                v[b] = w;
            }
        }
    } lut;
    auto run = [&](uint64_t b0, uint64_t b1) {  // whole bytes [b0, b1) -> characters 4 b0 ..
        for (uint64_t i = b0; i < b1; i++) memcpy(out + 4 * i, &lut.v[codes[i]], 4);
    };
    const uint64_t full = n / 4;
    const unsigned nt = full >= (1ull << 20) ? std::max(1u, std::min(16u, std::thread::hardware_concurrency())) : 1u;
    if (nt > 1) {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nt; t++) th.emplace_back(run, full * t / nt, full * (t + 1) / nt);
        for (auto &x : th) x.join();
    } else {
        run(0, full);
    }
    for (uint64_t c = 4 * full; c < n; c++) out[c] = "ACGT"[(codes[full] >> (2 * (c & 3))) & 3];
}

extern "C" {

int ec_session_create(ec_session **out, int device) {
    if (!out) {
        set_error("null out");
        return EC_ERR_ARG;
    }
    int n = 0;
    EC_HIP(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) {
        set_error("device %d not in [0,%d)", device, n);
        return EC_ERR_ARG;
    }
    EC_HIP(hipSetDevice(device));
    ec_session *s = new ec_session();
    s->device = device;
    if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) {
        delete s;
        set_error("hipStreamCreate failed");
        return EC_ERR_HIP;
    }
    s->own_stream = true;
    *out = s;
    return EC_OK;
}

int ec_session_set_stream(ec_session *s, void *hip_stream) {
    if (!s) return EC_ERR_ARG;
    EC_HIP(hipSetDevice(s->device));
    if (hip_stream == EC_OWN_STREAM) {
        if (!s->own_stream) {
            EC_HIP(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
            s->own_stream = true;
        }
        return EC_OK;
    }
    if (s->own_stream && s->stream) {
        (void)host_sync(s, s->stream);
        hipStreamDestroy(s->stream);
    }
    s->own_stream = false;
    s->stream = (hipStream_t)hip_stream;  // NULL: the null stream
    return EC_OK;
}

uint64_t ec_session_bytes(ec_session *s) {
    uint64_t n = 0;
    if (s) for_each_buf(s, [&](DevBuf &b) { n += b.cap; });
    return n;
}

int ec_session_trim(ec_session *s, uint64_t min_bytes) {
    if (!s) return EC_ERR_ARG;
    EC_HIP(hipSetDevice(s->device));
    if (s->stream) EC_HIP(hipStreamSynchronize(s->stream));
    if (s->ostream) EC_HIP(hipStreamSynchronize(s->ostream));
    if (s->cstream) EC_HIP(hipStreamSynchronize(s->cstream));
    for_each_buf(s, [&](DevBuf &b) {
        if (b.cap >= min_bytes && &b != &s->scal) b.release();
    });
    // no device state survives: the next call starts from its inputs (results already copied to
    // host memory stay fetchable)
    // (whatever min_bytes released: a trim always drops the held records and emitted runs too)
    drop_device_state(s, "ec_session_trim released the assembly's device state");
    s->n_dense = 0;
    s->skspec.valid = false;
    s->jlspec.valid = s->jlspec.queued = false;  // (its capacities are those of released buffers)
    s->pipe.active = false;
    return EC_OK;
}

int ec_mem_stats(uint64_t *held, uint64_t *peak, int reset) {
    if (held) *held = g_hbm_held.load();
    if (peak) *peak = g_hbm_peak.load();
    if (reset) g_hbm_peak.store(g_hbm_held.load());
    return EC_OK;
}

int ec_session_destroy(ec_session *s) {
    if (!s) return EC_OK;
    hipSetDevice(s->device);
    // every stream that may still copy into / out of the session's buffers (the speculative
    // contig copy on ostream, staged batches on cstream) drains before anything is released
    if (s->stream) hipStreamSynchronize(s->stream);
    if (s->ostream) hipStreamSynchronize(s->ostream);
    if (s->cstream) hipStreamSynchronize(s->cstream);
    if (s->events) {
        for (auto &e : s->ev) hipEventDestroy(e);
        for (auto &e : s->kev) hipEventDestroy(e);
    }
    if (s->rd_ev) hipEventDestroy(s->rd_ev);
    for (auto &e : s->oev)
        if (e) hipEventDestroy(e);
    for (auto &e : s->pipe.ev) hipEventDestroy(e);
    for (auto &sl : s->stg) {
        for (auto &e : sl.pipe.ev) hipEventDestroy(e);
        if (sl.free_ev) hipEventDestroy(sl.free_ev);
    }
    if (s->ostream) hipStreamDestroy(s->ostream);
    if (s->cstream) hipStreamDestroy(s->cstream);
    if (s->own_stream && s->stream) hipStreamDestroy(s->stream);
    delete s;  // (its device and pinned buffers free themselves: session.h)
    return EC_OK;
}

int ec_assemble_device(ec_session *s, const uint8_t *d_reads, const uint64_t *d_offsets, uint64_t nreads, int k,
                       int limit, unsigned flags) {
    if (!s || (!d_offsets)) {
        set_error("null session/offsets");
        return EC_ERR_ARG;
    }
    return assemble(s, d_reads, d_offsets, nreads, k, limit, flags);
}

int ec_assemble_host(ec_session *s, const uint8_t *reads, uint64_t nbytes, const uint64_t *offsets, uint64_t nreads,
                     int k, int limit, unsigned flags) {
    refresh_knobs();
    if (!s || !offsets || (nbytes && !reads)) {
        set_error("null argument");
        return EC_ERR_ARG;
    }
    EC_CHECK(check_offsets(offsets, nreads, nbytes));
    EC_HIP(hipSetDevice(s->device));
    EC_CHECK(s->h_reads.ensure(nbytes + 16));
    EC_CHECK(s->h_offsets.ensure((nreads + 1) * 8));
    // chunked copies (reads and offsets) on the copy stream, the partition of the reads that
    // have arrived overlapping the copies of the rest (s->pipe)
    EC_CHECK(pipe_plan(s, s->pipe, nbytes, 0, offsets, nreads, 0));
    auto &pp = s->pipe;
    pp.packed = false;
    pp.first_len = nreads ? offsets[1] - offsets[0] : 0;
    pp.ascii = s->h_reads.as<uint8_t>();
    for (int c = 0; c < pp.nchunks; c++) {
        if (pp.bhi[c] > pp.blo[c])
            EC_HIP(hipMemcpyAsync(s->h_reads.as<uint8_t>() + pp.blo[c], reads + pp.blo[c], pp.bhi[c] - pp.blo[c],
                                  hipMemcpyHostToDevice, s->cstream));
        EC_CHECK(pipe_copy_offsets(s, pp, c, offsets, s->h_offsets.as<uint64_t>()));
        EC_HIP(hipEventRecord(pp.ev[c], s->cstream));
    }
    return assemble_piped(s, s->h_offsets.as<uint64_t>(), nreads, k, limit, flags);
}

int ec_assemble_packed_host(ec_session *s, const uint8_t *codes, uint64_t nbases, const uint64_t *offsets,
                            uint64_t nreads, uint32_t read_len, const uint64_t *exc_pos, const uint8_t *exc_byte,
                            uint64_t n_exc, int k, int limit, unsigned flags) {
    refresh_knobs();
    if (!s) {
        set_error("null session");
        return EC_ERR_ARG;
    }
    if (s->stg_n) {
        set_error("staged batches pending (ec_assemble_staged first)");
        return EC_ERR_STATE;
    }
    EC_CHECK(check_packed(codes, nbases, offsets, nreads, read_len, exc_pos, exc_byte, n_exc));
    EC_HIP(hipSetDevice(s->device));
    EC_CHECK(s->h_reads.ensure(nbases + 16));
    EC_CHECK(stage_packed(s, s->pipe, s->p_codes, s->p_exc, s->h_offsets, nullptr, codes, nbases, offsets, nreads,
                          read_len, exc_pos, exc_byte, n_exc));
    return assemble_piped(s, s->h_offsets.as<uint64_t>(), nreads, k, limit, flags);
}

int ec_stage_packed_host(ec_session *s, const uint8_t *codes, uint64_t nbases, const uint64_t *offsets,
                         uint64_t nreads, uint32_t read_len, const uint64_t *exc_pos, const uint8_t *exc_byte,
                         uint64_t n_exc) {
    refresh_knobs();
    if (!s) {
        set_error("null session");
        return EC_ERR_ARG;
    }
    if (s->stg_n >= 2) {
        set_error("two batches already staged (ec_assemble_staged first)");
        return EC_ERR_STATE;
    }
    EC_CHECK(check_packed(codes, nbases, offsets, nreads, read_len, exc_pos, exc_byte, n_exc));
    EC_HIP(hipSetDevice(s->device));
    auto &sl = s->stg[(s->stg_head + s->stg_n) & 1];
    if (!sl.free_ev) {  // first use: free once the session stream's current work is done
        EC_HIP(hipEventCreateWithFlags(&sl.free_ev, hipEventDisableTiming));
        EC_HIP(hipEventRecord(sl.free_ev, s->stream));
    }
    EC_CHECK(stage_packed(s, sl.pipe, sl.codes, sl.exc, sl.off, sl.free_ev, codes, nbases, offsets, nreads, read_len,
                          exc_pos, exc_byte, n_exc));
    sl.nreads = nreads;
    sl.nbases = nbases;
    s->stg_n++;
    return EC_OK;
}

int ec_assemble_staged(ec_session *s, int k, int limit, unsigned flags) {
    refresh_knobs();
    if (!s) {
        set_error("null session");
        return EC_ERR_ARG;
    }
    if (!s->stg_n) {
        set_error("no staged batch (ec_stage_packed_host)");
        return EC_ERR_STATE;
    }
    EC_HIP(hipSetDevice(s->device));
    auto &sl = s->stg[s->stg_head];
    int rc = s->h_reads.ensure(sl.nbases + 16);
    if (rc == EC_OK) {
        std::swap(s->pipe, sl.pipe);
        rc = assemble_piped(s, sl.off.as<uint64_t>(), sl.nreads, k, limit, flags);
        std::swap(s->pipe, sl.pipe);
    }
    // the slot is free for the next staged batch once this call's kernels are done with it
    // (drained on every return, so also after a failure)
    if (sl.pipe.done < sl.pipe.nchunks) {  // (a failure before any chunk was consumed)
        for (int c = 0; c < sl.pipe.nchunks; c++) hipStreamWaitEvent(s->stream, sl.pipe.ev[c], 0);
    }
    hipEventRecord(sl.free_ev, s->stream);
    s->stg_head ^= 1;
    s->stg_n--;
    return rc;
}

int ec_get_stats(ec_session *s, ec_stats *out) {
    if (!s || !out) return EC_ERR_ARG;
    if (!s->stats_ok) {
        set_error("no successful call in this session");
        return EC_ERR_STATE;
    }
    *out = s->stats;
    return EC_OK;
}

int ec_spec_counts(ec_session *s, uint64_t out[4]) {
    if (!s || !out) return EC_ERR_ARG;
    for (int i = 0; i < 4; i++) out[i] = s->spec_cnt[i];
    return EC_OK;
}

const char *ec_stage_name(int stage) {
    static const char *names[EC_NSTAGES] = {"prescan", "count", "compact", "links", "rank", "starts", "emit", "gfa"};
    return (stage >= 0 && stage < EC_NSTAGES) ? names[stage] : "?";
}

int ec_copy_contigs(ec_session *s, char *chars, uint64_t *offsets) {
    if (!s) return EC_ERR_ARG;
    if (!s->have) {
        set_error("no successful assembly in this session");
        return EC_ERR_STATE;
    }
    if (chars && s->nchars_host) {
        if (s->chars_packed) unpack_codes(reinterpret_cast<const uint8_t *>(s->h_chars.data()), s->nchars_host, chars);
        else memcpy(chars, s->h_chars.data(), s->nchars_host);
    }
    if (offsets) memcpy(offsets, s->h_coff.data(), s->h_coff.size() * 8);
    return EC_OK;
}

int ec_copy_links(ec_session *s, uint64_t *link_offsets, int64_t *links) {
    if (!s) return EC_ERR_ARG;
    if (!s->have) {
        set_error("no successful assembly in this session");
        return EC_ERR_STATE;
    }
    if (s->links_compact) {  // (phase_graph's transfer form: widened here)
        if (link_offsets) {
            uint64_t o = 0;
            const size_t n2 = s->h_lc8.size();
            for (size_t i = 0; i < n2; i++) {
                link_offsets[i] = o;
                o += s->h_lc8[i];
            }
            link_offsets[n2] = o;
        }
        if (links)
            for (size_t i = 0; i < s->h_links32.size(); i++) links[i] = (int64_t)s->h_links32[i];
        return EC_OK;
    }
    if (link_offsets) memcpy(link_offsets, s->h_loff.data(), s->h_loff.size() * 8);
    if (links && !s->h_links.empty()) memcpy(links, s->h_links.data(), s->h_links.size() * 8);
    return EC_OK;
}

int ec_copy_dict(ec_session *s, char *kmers, uint32_t *counts) {
    if (!s) return EC_ERR_ARG;
    if (!s->have || !s->want_dict) {
        set_error("ec_copy_dict needs a successful ec_assemble_* with EC_FLAG_WANT_DICT");
        return EC_ERR_STATE;
    }
    const unsigned int U = (unsigned int)s->stats.n_solid;
    const unsigned int N = 2 * U;
    const unsigned B = 256;
    if (!U) return EC_OK;
    hipStream_t st = s->stream;
    EC_HIP(hipSetDevice(s->device));
    Scalars *dsc = s->scal.as<Scalars>();
    EC_HIP(hipMemsetAsync(&dsc->ndict, 0, 4, st));
    k_dict_items<<<grid_for(N, B), B, 0, st>>>(s->upal.as<uint8_t>(), s->dfc.as<unsigned long long>(),
                                              s->dft.as<unsigned long long>(), N, s->skeys.as<unsigned long long>(),
                                              s->svals.as<unsigned int>(), &dsc->ndict);
    unsigned int nd = 0;
    EC_CHECK(d2h(s, &nd, &dsc->ndict, 4, st));
    EC_CHECK(host_sync(s, st));
    EC_CHECK(sort_pairs(s, s->skeys.as<unsigned long long>(), s->skeys2.as<unsigned long long>(),
                        s->svals.as<unsigned int>(), s->svals2.as<unsigned int>(), nd));
    EC_CHECK(s->dchars.ensure((size_t)nd * s->k));
    EC_CHECK(s->dcounts.ensure((size_t)nd * 4));
    std::unique_lock<std::mutex> xlock(g_xmu, std::defer_lock);
    if (s->xalpha) {  // (c_xa may hold another session's alphabet by now)
        xlock.lock();
        EC_CHECK(x_upload(s));
        k_dict_render<OpsX><<<grid_for(nd, B), B, 0, st>>>(s->svals2.as<unsigned int>(), nd, s->dkey.as<K128>(),
                                                          s->dcnt.as<unsigned int>(), s->k, s->dchars.as<char>(),
                                                          s->dcounts.as<unsigned int>());
    } else if (s->k > 32)
        k_dict_render<OpsW><<<grid_for(nd, B), B, 0, st>>>(s->svals2.as<unsigned int>(), nd, s->dkey.as<K128>(),
                                                          s->dcnt.as<unsigned int>(), s->k, s->dchars.as<char>(),
                                                          s->dcounts.as<unsigned int>());
    else
        k_dict_render<Ops64><<<grid_for(nd, B), B, 0, st>>>(s->svals2.as<unsigned int>(), nd,
                                                           s->dkey.as<unsigned long long>(), s->dcnt.as<unsigned int>(),
                                                           s->k, s->dchars.as<char>(), s->dcounts.as<unsigned int>());
    if (kmers) EC_CHECK(d2h(s, kmers, s->dchars.p, (size_t)nd * s->k, st));
    if (counts) EC_CHECK(d2h(s, counts, s->dcounts.p, (size_t)nd * 4, st));
    EC_CHECK(host_sync(s, st));
    return EC_OK;
}


// ---- sharded (multi-GPU) building blocks ---------------------------------------------------
int ec_count_shard(ec_session *s, const uint8_t *d_reads, const uint64_t *d_offsets, uint64_t nreads,
                   uint64_t read_base, int k, unsigned flags) {
    if (!s || !d_offsets) {
        set_error("null session/offsets");
        return EC_ERR_ARG;
    }
    EC_CHECK(begin_call(s, k, flags));
    if (read_base + nreads > (1ull << 32)) {
        set_error("global read ids reach %llu >= 2^32", (unsigned long long)(read_base + nreads));
        return EC_ERR_CAPACITY;
    }
    unsigned int U = 0;
    s->no_index = true;
    int rc = EC_OK;
    // the shard is counted with shard-relative read ids (so every rank qualifies for the
    // super-k-mer path's 32-bit positions, count_sk2.h); first events are events
    // (read << 32) | window, so the export adds read_base << 32 to every real event
    if (k > 32) {
        SolidIndexW sidx{};
        rc = phase_count_w(s, d_reads, d_offsets, nreads, 0, k, LLONG_MIN, U, sidx);
    } else {
        SolidIndex sidx{};
        rc = phase_count(s, d_reads, d_offsets, nreads, 0, k, LLONG_MIN, flags, U, sidx);
    }
    s->no_index = false;
    EC_CHECK(rc);
    s->clip_why = CLIP_WHY_STEPWISE;
    s->shard_base = read_base;
    s->n_dense = U;
    s->dense_ok = true;
    collect_timing(s);
    s->stats_ok = true;
    return EC_OK;
}

int ec_session_set_owner_rule(ec_session *s, int rule) {
    if (!s || rule < 0 || rule > 1) {
        set_error("bad owner rule %d", rule);
        return EC_ERR_ARG;
    }
    if (rule != s->owner_rule) s->own_valid = false;
    s->owner_rule = rule;
    return EC_OK;
}

int ec_export_by_owner(ec_session *s, int nowners, void *d_out, uint64_t *owner_counts) {
    return ec_export_by_owner_ex(s, nowners, d_out, owner_counts, 0, nullptr);
}

int ec_export_by_owner_ex(ec_session *s, int nowners, void *d_out, uint64_t *owner_counts, int compact,
                          int *lf_bits) {
    refresh_knobs();
    if (!s || nowners < 1 || nowners > MAX_OWNERS || !owner_counts) {
        set_error("bad ec_export_by_owner arguments (nowners=%d)", nowners);
        return EC_ERR_ARG;
    }
    if (!s->dense_ok) {
        set_error("ec_export_by_owner: no counted or merged records (ec_count_shard / ec_merge_owned)");
        return EC_ERR_STATE;
    }
    EC_HIP(hipSetDevice(s->device));
    hipStream_t st = s->stream;
    const unsigned B = 256;
    const unsigned int n = s->n_dense;
    const unsigned int nblk = (unsigned int)std::max<uint64_t>((n + OWN_CHUNK - 1) / OWN_CHUNK, 1);
    const size_t nbh = (size_t)nowners * nblk;
    EC_CHECK(s->ocnt.ensure(2 * nbh * 4));
    unsigned int *bh = s->ocnt.as<unsigned int>(), *bhi = bh + nbh;
    const bool wide = s->k > 32;
    OwnerFn own = owner_fn(s->k);
    if (s->owner_rule == 1) own.sk = 0, own.wk = 0;  // key-hash owners (a skewed minimizer distribution)
    EC_CHECK(s->mbid.ensure(std::max<uint64_t>(n, 1) * 4));  // owner of each record (free until a merge)
    EC_CHECK(s->ocnt.ensure(2 * nbh * 4 + 16));
    bh = s->ocnt.as<unsigned int>(), bhi = bh + nbh;
    unsigned int *evmax = bhi + nbh;  // largest shard-relative read id / position of the events
    unsigned int *oid = s->mbid.as<unsigned int>();
    const bool reuse = s->own_valid && s->own_rule == s->owner_rule && s->own_nowners == nowners && s->own_n == n &&
                       s->own_nblk == nblk;
    if (!reuse) {
        s->own_hi.assign(nbh + 2, 0u);
        if (n) {
            EC_HIP(hipMemsetAsync(evmax, 0, 8, st));
            if (wide)
                k_owner_hist<K128><<<nblk, B, 0, st>>>(s->dkey.as<K128>(), n, nowners, nblk, bh, own, oid,
                                                       s->dfc.as<unsigned long long>(), s->dft.as<unsigned long long>(),
                                                       evmax);
            else
                k_owner_hist<unsigned long long><<<nblk, B, 0, st>>>(s->dkey.as<unsigned long long>(), n, nowners, nblk,
                                                                    bh, own, oid, s->dfc.as<unsigned long long>(),
                                                                    s->dft.as<unsigned long long>(), evmax);
            EC_CHECK(scan_incl_u32(s, bh, bhi, nbh));
            EC_CHECK(d2h(s, s->own_hi.data(), bhi, nbh * 4 + 8, st));  // (+ the event maxima)
        }
        if (compact && n) EC_CHECK(host_sync(s, st));  // (the event widths choose the record format)
    }
    int lfb = -1;  // compact records: bits of the window position (the read id above them), else full
    if (compact && lf_bits) {
        const unsigned int mr = n ? s->own_hi[nbh] : 0u, ml = n ? s->own_hi[nbh + 1] : 0u;
        int lb = 1, rb = 0;
        while (lb < 31 && (ml >> lb)) lb++;
        while (rb < 32 && (mr >> rb)) rb++;
        // (the all-ones code is "no event": it must stay out of range)
        if (lb + rb <= 32 && !(lb + rb == 32 && mr == (0xFFFFFFFFu >> lb) && ml == (1u << lb) - 1)) lfb = lb;
        *lf_bits = lfb;
    }
    if (n && d_out && lfb >= 0) {  // compact records (shard-relative events)
        if (wide)
            k_owner_scatter_c<K128><<<nblk, B, 0, st>>>(s->dkey.as<K128>(), s->dcnt.as<unsigned int>(),
                                                        s->dfc.as<unsigned long long>(), s->dft.as<unsigned long long>(),
                                                        n, nowners, nblk, bhi, reinterpret_cast<CRecW *>(d_out), lfb, oid);
        else
            k_owner_scatter_c<unsigned long long><<<nblk, B, 0, st>>>(
                s->dkey.as<unsigned long long>(), s->dcnt.as<unsigned int>(), s->dfc.as<unsigned long long>(),
                s->dft.as<unsigned long long>(), n, nowners, nblk, bhi, reinterpret_cast<CRec *>(d_out), lfb, oid);
    } else if (n && d_out) {  // the scatter is queued before the host waits for the owner counts
        if (wide)
            k_owner_scatter<K128><<<nblk, B, 0, st>>>(s->dkey.as<K128>(), s->dcnt.as<unsigned int>(),
                                                      s->dfc.as<unsigned long long>(), s->dft.as<unsigned long long>(),
                                                      n, nowners, nblk, bhi, reinterpret_cast<AggW *>(d_out),
                                                      s->shard_base << 32, oid);
        else
            k_owner_scatter<unsigned long long><<<nblk, B, 0, st>>>(
                s->dkey.as<unsigned long long>(), s->dcnt.as<unsigned int>(), s->dfc.as<unsigned long long>(),
                s->dft.as<unsigned long long>(), n, nowners, nblk, bhi, reinterpret_cast<Agg *>(d_out),
                s->shard_base << 32, oid);
    }
    EC_CHECK(host_sync(s, st));
    s->own_valid = true, s->own_rule = s->owner_rule, s->own_nowners = nowners, s->own_n = n, s->own_nblk = nblk;
    unsigned long long prev = 0;
    for (int i = 0; i < nowners; i++) {
        const unsigned long long end = n ? s->own_hi[(size_t)(i + 1) * nblk - 1] : 0ull;
        owner_counts[i] = end - prev;
        prev = end;
    }
    return EC_OK;
}

}  // extern "C"

// the owner merge; xin: k <= 32 records read in place (decode: the decoded copy, for the HBM table)
int merge_owned_impl(ec_session *s, const void *d_records, uint64_t n, int k, int limit, unsigned flags,
                     const XIn *xin = nullptr, const std::function<int(const Agg *&)> &decode = nullptr) {
    if (!s || (n && !d_records)) {
        set_error("null argument");
        return EC_ERR_ARG;
    }
    EC_CHECK(begin_call(s, k, flags));
    unsigned int U = 0;
    s->no_index = true;
    int rc = EC_OK;
    if (k > 32) {
        SolidIndexW sidx{};
        rc = phase_merge_w(s, reinterpret_cast<const AggW *>(d_records), n, (long long)limit, U, sidx);
    } else {
        SolidIndex sidx{};
        rc = phase_merge(s, reinterpret_cast<const Agg *>(d_records), n, (long long)limit, U, sidx, xin, decode);
    }
    s->no_index = false;
    EC_CHECK(rc);
    s->clip_why = CLIP_WHY_STEPWISE;
    s->n_dense = U;
    s->dense_ok = true;
    collect_timing(s);
    s->stats_ok = true;
    return EC_OK;
}

extern "C" {

int ec_merge_owned(ec_session *s, const void *d_records, uint64_t n, int k, int limit, unsigned flags) {
    return merge_owned_impl(s, d_records, n, k, limit, flags);
}

// the merge of records received from nsrc ranks (ec_export_by_owner_ex: compact or full per
// source) -- decoded to exchange records with global events, then ec_merge_owned
int ec_merge_owned_from(ec_session *s, const void *d_records, int nsrc, const uint64_t *src_bytes,
                        const int64_t *src_read_base, const int32_t *src_lf_bits, int k, int limit, unsigned flags) {
    if (!s || nsrc < 1 || nsrc > MAX_OWNERS || !src_bytes || !src_read_base || !src_lf_bits || k < 1 || k > EC_MAX_K) {
        set_error("ec_merge_owned_from: bad arguments");
        return EC_ERR_ARG;
    }
    const size_t full = k > 32 ? sizeof(AggW) : sizeof(Agg), comp = k > 32 ? sizeof(CRecW) : sizeof(CRec);
    std::vector<unsigned long long> hoff(2 * (size_t)nsrc + 2);
    std::vector<long long> hb(nsrc);
    std::vector<int> hl(nsrc);
    unsigned long long bsum = 0, rsum = 0;
    for (int q = 0; q < nsrc; q++) {
        const size_t rb = src_lf_bits[q] >= 0 ? comp : full;
        if (src_bytes[q] % rb || src_lf_bits[q] > 31) {
            set_error("ec_merge_owned_from: source %d sends %llu bytes of %zu-B records", q,
                      (unsigned long long)src_bytes[q], rb);
            return EC_ERR_ARG;
        }
        hoff[q] = bsum;
        hoff[nsrc + 1 + q] = rsum;
        bsum += src_bytes[q];
        rsum += src_bytes[q] / rb;
        hb[q] = src_read_base[q];
        hl[q] = src_lf_bits[q];
    }
    hoff[nsrc] = bsum;
    hoff[2 * (size_t)nsrc + 1] = rsum;
    if (bsum && !d_records) {
        set_error("null records");
        return EC_ERR_ARG;
    }
    EC_HIP(hipSetDevice(s->device));
    hipStream_t st = s->stream;
    const size_t mbytes = hoff.size() * 8 + (size_t)nsrc * 12;
    EC_CHECK(s->xrec.ensure(std::max<uint64_t>(rsum, 1) * full + mbytes + 64));
    uint8_t *meta = s->xrec.as<uint8_t>() + std::max<uint64_t>(rsum, 1) * full;
    unsigned long long *doff = reinterpret_cast<unsigned long long *>(meta);
    long long *dbase = reinterpret_cast<long long *>(doff + hoff.size());
    int *dlfb = reinterpret_cast<int *>(dbase + nsrc);
    // one H2D copy from page-locked staging (three pageable copies cost ~0.1 ms a call)
    EC_HIP(hipStreamSynchronize(st));  // (the staging of an earlier call has been read)
    EC_CHECK(s->hmeta.resize(mbytes));
    memcpy(s->hmeta.data(), hoff.data(), hoff.size() * 8);
    memcpy(s->hmeta.data() + hoff.size() * 8, hb.data(), (size_t)nsrc * 8);
    memcpy(s->hmeta.data() + hoff.size() * 8 + (size_t)nsrc * 8, hl.data(), (size_t)nsrc * 4);
    EC_HIP(hipMemcpyAsync(doff, s->hmeta.data(), mbytes, hipMemcpyHostToDevice, st));
    if (k <= 32 && rsum) {
        // k <= 32: the merge reads the received records in place; the decoded copy only for the
        // HBM-table fallback (a bucket past its LDS table, or EC_FLAG_GENERAL)
        const XIn xin{static_cast<const uint8_t *>(d_records), doff, doff + nsrc + 1, dbase, dlfb, nsrc};
        auto decode = [&](const Agg *&out) -> int {
            k_uncompact<unsigned long long><<<grid_for(rsum, 256), 256, 0, s->stream>>>(
                static_cast<const uint8_t *>(d_records), doff, doff + nsrc + 1, dbase, dlfb, nsrc, rsum, s->xrec.as<Agg>());
            out = s->xrec.as<Agg>();
            return EC_OK;
        };
        return merge_owned_impl(s, s->xrec.p, rsum, k, limit, flags, &xin, decode);
    }
    if (rsum)  // (k > 32: the merge reads a decoded copy)
        k_uncompact<K128><<<grid_for(rsum, 256), 256, 0, st>>>(static_cast<const uint8_t *>(d_records), doff,
                                                              doff + nsrc + 1, dbase, dlfb, nsrc, rsum,
                                                              s->xrec.as<AggW>());
    return ec_merge_owned(s, s->xrec.p, rsum, k, limit, flags);
}

int ec_compact_record_bytes(int k) { return k > 32 ? (int)sizeof(CRecW) : (int)sizeof(CRec); }

int ec_export_dense(ec_session *s, void *d_out) {
    if (!s) return EC_ERR_ARG;
    if (!s->dense_ok) {
        set_error("ec_export_dense: no counted or merged records (ec_count_shard / ec_merge_owned)");
        return EC_ERR_STATE;
    }
    EC_HIP(hipSetDevice(s->device));
    const unsigned int n = s->n_dense;
    if (n && d_out) {
        if (s->k > 32)
            k_export_dense<K128><<<grid_for(n, 256), 256, 0, s->stream>>>(
                s->dkey.as<K128>(), s->dcnt.as<unsigned int>(), s->dfc.as<unsigned long long>(),
                s->dft.as<unsigned long long>(), n, reinterpret_cast<AggW *>(d_out), s->shard_base << 32);
        else
            k_export_dense<unsigned long long><<<grid_for(n, 256), 256, 0, s->stream>>>(
                s->dkey.as<unsigned long long>(), s->dcnt.as<unsigned int>(), s->dfc.as<unsigned long long>(),
                s->dft.as<unsigned long long>(), n, reinterpret_cast<Agg *>(d_out), s->shard_base << 32);
        EC_CHECK(host_sync(s, s->stream));
    }
    return EC_OK;
}

uint64_t ec_dense_count(ec_session *s) { return s ? s->n_dense : 0; }

int ec_merge_owned_export(ec_session *s, const void *d_records, uint64_t n, int k, int limit, unsigned flags,
                          void *d_out) {
    EC_CHECK(ec_merge_owned(s, d_records, n, k, limit, flags));
    return ec_export_dense(s, d_out);
}

int ec_assemble_from_solid(ec_session *s, const void *d_records, uint64_t n, int k, unsigned flags) {
    if (!s || (n && !d_records)) {
        set_error("null argument");
        return EC_ERR_ARG;
    }
    EC_CHECK(begin_call(s, k, flags));
    unsigned int U = 0;
    if (k > 32) {
        SolidIndexW sidx{};
        EC_CHECK(phase_merge_w(s, reinterpret_cast<const AggW *>(d_records), n, LLONG_MIN, U, sidx));
        return phase_graph<OpsW>(s, k, U, sidx);
    }
    // the gathered keys are distinct; the bucketed merge (sort by bucket + LDS tables) is also
    // the fastest loader: measured 0.42 ms at 4.6 M keys against 0.60 ms for per-key CAS
    // inserts into the HBM sub-table (random-address atomics)
    SolidIndex sidx{};
    EC_CHECK(phase_merge(s, reinterpret_cast<const Agg *>(d_records), n, LLONG_MIN, U, sidx));
    return phase_graph<Ops64>(s, k, U, sidx);
}

int ec_record_bytes(int k) { return k > 32 ? (int)sizeof(AggW) : (int)sizeof(Agg); }

int ec_graph_load(ec_session *s, const void *d_records, uint64_t n, int k, unsigned flags) {
    if (!s || (n && !d_records)) {
        set_error("null argument");
        return EC_ERR_ARG;
    }
    s->graph_loaded = false;
    // the owner merge's bucket marks (this rank's segment of the set loaded here) outlive the load
    const uint64_t marks = s->seg_marks;
    EC_CHECK(begin_call(s, k, flags));
    s->seg_marks = marks;
    unsigned int U = 0;
    if (k > 32)
        EC_CHECK(phase_load_det_w(s, reinterpret_cast<const AggW *>(d_records), n, U, s->gidxw));
    else
        EC_CHECK(phase_load_det(s, reinterpret_cast<const Agg *>(d_records), n, U, s->gidx));
    EC_CHECK(check_node_ids(U));
    s->n_dense = U;
    s->graph_loaded = true;
    s->clip_why = CLIP_WHY_STEPWISE;
    collect_timing(s);
    s->stats_ok = true;
    return EC_OK;
}

int ec_graph_links_part(ec_session *s, uint64_t lo, uint64_t hi, uint32_t *d_succ) {
    refresh_knobs();
    if (!s || !s->graph_loaded || s->placed || lo > hi || hi > s->n_dense || (hi > lo && !d_succ)) {
        set_error("ec_graph_links_part: no loaded solid set or bad range [%llu, %llu)", (unsigned long long)lo,
                  (unsigned long long)hi);
        return EC_ERR_ARG;
    }
    EC_HIP(hipSetDevice(s->device));
    if (hi > lo) {
        const uint64_t n = 2 * (hi - lo);
        if (s->k > 32)
            k_links_part<OpsW, SolidIndexW><<<grid_for(n, 256), 256, 0, s->stream>>>(
                s->gidxw, s->dkey.as<K128>(), (unsigned int)lo, (unsigned int)hi, s->k, d_succ);
        else
            k_links_part<Ops64, SolidIndex><<<grid_for(n, 256), 256, 0, s->stream>>>(
                s->gidx, s->dkey.as<unsigned long long>(), (unsigned int)lo, (unsigned int)hi, s->k, d_succ);
        EC_HIP(hipGetLastError());
    }
    EC_CHECK(host_sync(s, s->stream));
    return EC_OK;
}

int ec_graph_load_links(ec_session *s, const void *d_records, uint64_t n, int k, unsigned flags, uint64_t lo,
                        uint64_t hi, uint32_t *d_succ) {
    EC_CHECK(ec_graph_load(s, d_records, n, k, flags));
    return ec_graph_links_part(s, lo, hi, d_succ);
}

int ec_graph_finish(ec_session *s, const uint32_t *d_succ, unsigned flags) {
    if (!s || !s->graph_loaded || s->placed || (s->n_dense && !d_succ)) {
        set_error("ec_graph_finish: no loaded solid set");
        return EC_ERR_ARG;
    }
    const unsigned int U = (unsigned int)s->n_dense;
    const ec_stats keep = s->stats;
    EC_CHECK(begin_call(s, s->k, flags));
    s->stats = keep;
    for (float &v : s->stats.stage_ms) v = 0.0f;
    for (float &v : s->stats.kernel_ms) v = 0.0f;
    s->graph_loaded = false;
    if (s->k > 32) return phase_graph<OpsW>(s, s->k, U, s->gidxw, d_succ);
    return phase_graph<Ops64>(s, s->k, U, s->gidx, d_succ);
}

// multi-GPU partitioned finish (see part_chains above); include/eulerhip.h
int ec_graph_chains_part(ec_session *s, uint64_t lo, uint64_t hi, const uint32_t *d_succ, void *d_super,
                         uint64_t *n_super) {
    refresh_knobs();
    if (!s || !s->graph_loaded || lo > hi || hi > s->n_dense || !n_super ||
        (hi > lo && !d_succ && !s->placed) ||
        (s->placed && (lo != s->seg_lo || hi != s->seg_lo + s->seg_Ur))) {
        set_error("ec_graph_chains_part: no loaded solid set or bad range [%llu, %llu)", (unsigned long long)lo,
                  (unsigned long long)hi);
        return EC_ERR_ARG;
    }
    EC_HIP(hipSetDevice(s->device));
    SuperRec *out = static_cast<SuperRec *>(d_super);
    return s->k > 32 ? part_chains<OpsW>(s, lo, hi, d_succ, out, n_super)
                     : part_chains<Ops64>(s, lo, hi, d_succ, out, n_super);
}

int ec_graph_rank_supers(ec_session *s, const void *d_supers, uint64_t n) {
    if (!s || !s->graph_loaded || s->part_stage < 1 || (n && !d_supers)) {
        set_error("ec_graph_rank_supers: no loaded solid set with ranked chains (ec_graph_chains_part)");
        return EC_ERR_ARG;
    }
    EC_HIP(hipSetDevice(s->device));
    return part_rank(s, static_cast<const SuperRec *>(d_supers), n);
}

int ec_graph_starts_part(ec_session *s, int have_supers, void *d_starts, uint64_t *n_starts) {
    if (!s || !s->graph_loaded || s->part_stage < 2 || !n_starts) {
        set_error("ec_graph_starts_part: no loaded solid set with ranked supers (ec_graph_rank_supers)");
        return EC_ERR_ARG;
    }
    EC_HIP(hipSetDevice(s->device));
    return part_starts(s, have_supers != 0, static_cast<StartRec *>(d_starts), n_starts);
}

// the records a step called with a NULL output counted (exact-size buffers)
static int take_pending(ec_session *s, int kind, const void *d_out, const char *what, uint64_t &n) {
    if (!s || s->hold.kind != kind || (s->hold.n && !d_out)) {
        set_error("%s: no pending records of this step (call it with a NULL output first)", what);
        return EC_ERR_STATE;
    }
    n = s->hold.n;
    s->hold.kind = 0;
    return hipSetDevice(s->device) == hipSuccess ? EC_OK : EC_ERR_HIP;
}

int ec_graph_place_copy(ec_session *s, void *d_jrecs) {
    uint64_t n = 0;
    EC_CHECK(take_pending(s, 1, d_jrecs, "ec_graph_place_copy", n));
    if (n) {
        if (s->k > 32)
            k_gather_recs<RecJ><<<grid_for(n, 256), 256, 0, s->stream>>>(s->jrec.as<RecJ>(), s->midx2.as<unsigned int>(), n,
                                                                      static_cast<RecJ *>(d_jrecs));
        else
            k_gather_recs<RecJ64><<<grid_for(n, 256), 256, 0, s->stream>>>(
                s->jrec.as<RecJ64>(), s->midx2.as<unsigned int>(), n, static_cast<RecJ64 *>(d_jrecs));
    }
    return host_sync(s, s->stream);
}

int ec_graph_chains_copy(ec_session *s, void *d_super) {
    uint64_t n = 0;
    if (s && s->hold.kind == 2 && !s->chain_scr) s->hold.kind = 0;  // (records gone: refused below)
    EC_CHECK(take_pending(s, 2, d_super, "ec_graph_chains_copy", n));
    return part_chains_copy(s, n, s->hold.ntiles, s->hold.planned, static_cast<SuperRec *>(d_super));
}

int ec_graph_starts_copy(ec_session *s, void *d_starts) {
    uint64_t n = 0;
    EC_CHECK(take_pending(s, 3, d_starts, "ec_graph_starts_copy", n));
    return part_starts_copy(s, n, static_cast<StartRec *>(d_starts));
}

int ec_graph_layout(ec_session *s, const void *d_starts, uint64_t n, uint64_t *n_chars) {
    if (!s || !s->graph_loaded || s->part_stage < 3 || !n_chars || (n && !d_starts)) {
        set_error("ec_graph_layout: no loaded solid set with its starts (ec_graph_starts_part)");
        return EC_ERR_ARG;
    }
    EC_HIP(hipSetDevice(s->device));
    return part_layout(s, static_cast<const StartRec *>(d_starts), n, n_chars);
}

int ec_graph_emit_part(ec_session *s, char *d_chars, void *d_ends) {
    if (!s || !s->graph_loaded || s->part_stage < 4 || (s->seg_nchars && !d_chars) || (s->seg_nc && !d_ends)) {
        set_error("ec_graph_emit_part: no layout");
        return EC_ERR_ARG;
    }
    EC_HIP(hipSetDevice(s->device));
    return s->k > 32 ? part_emit<OpsW>(s, d_chars, d_ends) : part_emit<Ops64>(s, d_chars, d_ends);
}

int ec_graph_collect(ec_session *s, const char *d_chars, const void *d_ends, uint64_t n_pal) {
    if (!s || !s->graph_loaded || s->part_stage < 4 || (s->seg_nchars && !d_chars) || (s->seg_nc && !d_ends) ||
        2 * n_pal > 2 * s->n_dense) {
        set_error("ec_graph_collect: no layout");
        return EC_ERR_ARG;
    }
    EC_HIP(hipSetDevice(s->device));
    return s->k > 32 ? part_collect<OpsW>(s, d_chars, d_ends, n_pal) : part_collect<Ops64>(s, d_chars, d_ends, n_pal);
}

int ec_graph_emit_runs(ec_session *s, uint64_t *nbytes) {
    if (!s || !s->graph_loaded || s->part_stage < 4 || !nbytes) {
        set_error("ec_graph_emit_runs: no layout");
        return EC_ERR_ARG;
    }
    EC_HIP(hipSetDevice(s->device));
    return s->k > 32 ? part_emit_runs<OpsW>(s, nbytes) : part_emit_runs<Ops64>(s, nbytes);
}

int ec_graph_copy_runs(ec_session *s, void *d_out) {
    if (!s || !d_out) {
        set_error("ec_graph_copy_runs: null argument");
        return EC_ERR_ARG;
    }
    if (!s->runs_ready || !s->graph_loaded) {
        set_error("ec_graph_copy_runs: no emitted runs (ec_graph_emit_runs)");
        return EC_ERR_STATE;
    }
    EC_HIP(hipSetDevice(s->device));
    return s->k > 32 ? part_copy_runs<OpsW>(s, d_out) : part_copy_runs<Ops64>(s, d_out);
}

int ec_graph_collect_runs(ec_session *s, const void *d_in, int nsrc, const uint64_t *src_bytes, uint64_t n_pal) {
    if (!s || !s->graph_loaded || s->part_stage < 4 || nsrc < 1 || !src_bytes || !d_in || n_pal > s->n_dense) {
        set_error("ec_graph_collect_runs: no layout or bad arguments");
        return EC_ERR_ARG;
    }
    EC_HIP(hipSetDevice(s->device));
    return s->k > 32 ? part_collect_runs<OpsW>(s, static_cast<const uint8_t *>(d_in), nsrc, src_bytes, n_pal)
                     : part_collect_runs<Ops64>(s, static_cast<const uint8_t *>(d_in), nsrc, src_bytes, n_pal);
}

int ec_end_record_bytes(int k) { return k > 32 ? 16 : 8; }
int ec_junction_record_bytes(int k) { return k > 32 ? (int)sizeof(RecJ) : (int)sizeof(RecJ64); }
int ec_link_record_bytes(void) { return (int)sizeof(LinkRec); }

}  // extern "C"

// ---- junction-partitioned graph (junction.h) ------------------------------------------------
// counting sort of n ids (bins 0..nbins-1) -> perm (midx2) and bin starts bstart[0..nbins]
int bin_sort(ec_session *s, const unsigned int *bid, uint64_t n, unsigned int nbins, unsigned long long *bstart) {
    EC_CHECK(s->midx2.ensure(std::max<uint64_t>(n, 1) * 4));
    if (!n) {
        EC_HIP(hipMemsetAsync(bstart, 0, (nbins + 1ull) * 8, s->stream));
        return EC_OK;
    }
    return cs_sort(s, bid, n, nbins, bstart, true);
}

template <typename K>
int graph_place(ec_session *s, uint64_t lo, uint64_t U, int nowners, void *d_out, uint64_t *owner_counts,
                uint64_t *n_pal) {
    using R = typename JRecOf<K>::R;
    using Ops = typename std::conditional<sizeof(K) == 8, Ops64, OpsW>::type;
    hipStream_t st = s->stream;
    const unsigned B = 256;
    Scalars *dsc = s->scal.as<Scalars>();
    const uint64_t Ur = s->n_dense, Uu = std::max<uint64_t>(U, 1);
    // (the dense arrays, the successors and the junction records -- a chains step's records among
    // them -- are rewritten: nothing held or ranked on them survives; loaded / placed again at the end)
    drop_step_state(s);
    s->graph_loaded = false;
    s->placed = false;
    s->dense_ok = false;
    // the merge's dense arrays [0, Ur) -> global ids [lo, lo + Ur) of U-sized arrays
    EC_CHECK(s->recs.ensure(std::max<uint64_t>(Ur, 1) * sizeof(K)));
    EC_CHECK(s->recs2.ensure(std::max<uint64_t>(Ur, 1) * 16));
    EC_CHECK(s->midx.ensure(std::max<uint64_t>(Ur, 1) * 4));
    unsigned long long *tfc = s->recs2.as<unsigned long long>(), *tft = tfc + Ur;
    if (Ur) {
        EC_HIP(hipMemcpyAsync(s->recs.p, s->dkey.p, Ur * sizeof(K), hipMemcpyDeviceToDevice, st));
        EC_HIP(hipMemcpyAsync(s->midx.p, s->dcnt.p, Ur * 4, hipMemcpyDeviceToDevice, st));
        EC_HIP(hipMemcpyAsync(tfc, s->dfc.p, Ur * 8, hipMemcpyDeviceToDevice, st));
        EC_HIP(hipMemcpyAsync(tft, s->dft.p, Ur * 8, hipMemcpyDeviceToDevice, st));
    }
    if (s->dkey.cap < Uu * sizeof(K) || s->dcnt.cap < Uu * 4 || s->dfc.cap < Uu * 8 || s->dft.cap < Uu * 8)
        EC_HIP(hipStreamSynchronize(st));  // (the ensure()s below free the copies' sources)
    EC_CHECK(s->dkey.ensure(Uu * sizeof(K)));
    EC_CHECK(s->dcnt.ensure(Uu * 4));
    EC_CHECK(s->dfc.ensure(Uu * 8));
    EC_CHECK(s->dft.ensure(Uu * 8));
    EC_CHECK(s->upal.ensure(Uu));
    EC_CHECK(s->succ.ensure(2 * Uu * 4));
    if (Ur) {
        EC_HIP(hipMemcpyAsync(s->dkey.as<K>() + lo, s->recs.p, Ur * sizeof(K), hipMemcpyDeviceToDevice, st));
        EC_HIP(hipMemcpyAsync(s->dcnt.as<unsigned int>() + lo, s->midx.p, Ur * 4, hipMemcpyDeviceToDevice, st));
        EC_HIP(hipMemcpyAsync(s->dfc.as<unsigned long long>() + lo, tfc, Ur * 8, hipMemcpyDeviceToDevice, st));
        EC_HIP(hipMemcpyAsync(s->dft.as<unsigned long long>() + lo, tft, Ur * 8, hipMemcpyDeviceToDevice, st));
        EC_HIP(hipMemsetAsync(s->succ.as<unsigned int>() + 2 * lo, 0xFF, 2 * Ur * 4, st));
    }
    EC_HIP(hipMemsetAsync(&dsc->npal, 0, 4, st));
    if (Ur)
        EC_CHECK(launch_upal<Ops>(st, s->dkey.as<K>() + lo, (unsigned int)Ur, s->k, s->upal.as<uint8_t>() + lo,
                                  &dsc->npal));
    // junction records routed to the junctions' owners (the keys' rule, shard.h OwnerFn)
    OwnerFn own = owner_fn(s->k);
    if (s->owner_rule == 1) own.sk = 0, own.wk = 0;
    JOwnerFn jown{};
    jown.sk = own.sk;
    if (own.sk) jown.mcj = sk_cfg(s->k - 1);
    jown.wj = own.wk ? s->k - 1 : 0;
    const uint64_t nslot = 4 * Ur;
    EC_CHECK(s->jrec.ensure(std::max<uint64_t>(nslot, 1) * sizeof(R)));
    EC_CHECK(s->joid.ensure(std::max<uint64_t>(nslot, 1) * 4));
    EC_CHECK(s->jseg.ensure(((size_t)nowners + 2) * 8));
    unsigned long long *ostart = s->jseg.as<unsigned long long>();
    if (Ur)
        k_junction_emit<K><<<grid_for(Ur, B), B, 0, st>>>(s->dkey.as<K>(), s->upal.as<uint8_t>(), (unsigned int)lo,
                                                         (unsigned int)Ur, s->k, jown, (unsigned int)nowners,
                                                         s->jrec.as<R>(), s->joid.as<unsigned int>());
    // owner-major order: counting sort by owner (NONE slots in the last bin, dropped)
    EC_CHECK(s->joid.ensure(std::max<uint64_t>(nslot, 1) * 4));
    if (nslot) k_none_to_bin<<<grid_for(nslot, B), B, 0, st>>>(s->joid.as<unsigned int>(), nslot, (unsigned int)nowners);
    EC_CHECK(bin_sort(s, s->joid.as<unsigned int>(), nslot, (unsigned int)nowners + 1, ostart));
    if (nslot && d_out)  // (NULL: counted only, ec_graph_place_copy gathers the owned records)
        k_gather_recs<R><<<grid_for(nslot, B), B, 0, st>>>(s->jrec.as<R>(), s->midx2.as<unsigned int>(), nslot,
                                                          static_cast<R *>(d_out));
    std::vector<unsigned long long> hs((size_t)nowners + 2);
    EC_CHECK(d2h(s, hs.data(), ostart, ((size_t)nowners + 2) * 8, st));
    unsigned int npal = 0;
    EC_CHECK(d2h(s, &npal, &dsc->npal, 4, st));
    EC_CHECK(host_sync(s, st));
    for (int r = 0; r < nowners; r++) owner_counts[r] = hs[r + 1] - hs[r];
    if (!d_out) s->hold = ec_session::Pending{1, hs[nowners], 0, false};
    *n_pal = npal;
    s->seg_lo = lo;
    s->seg_Ur = Ur;
    s->n_dense = (unsigned int)U;
    s->placed = true;
    s->graph_loaded = true;  // (the part_* steps' state: the placed segment)
    s->seg_n0 = 2 * lo;
    s->seg_n1 = 2 * (lo + Ur);
    return EC_OK;
}

// bin starts of n bin ids sorted ascending (bstart[b] = first index with id >= b, bstart[nb] = n)
__global__ void __launch_bounds__(256) k_sorted_starts(const unsigned int *key, uint64_t n, unsigned int nb,
                                                      unsigned long long *bstart) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const unsigned int kk = key[i];
        const long long prev = i ? (long long)key[i - 1] : -1ll;
        for (long long b = prev + 1; b <= (long long)kk; b++) bstart[b] = i;
        if (i + 1 == n)
            for (long long b = (long long)kk + 1; b <= (long long)nb; b++) bstart[b] = n;
    }
}
__global__ void __launch_bounds__(256) k_iota_u32(unsigned int *v, uint64_t n) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        v[i] = (unsigned int)i;
}

template <typename R>
int graph_join(ec_session *s, const R *d_recs, uint64_t n, int nowners, const uint64_t *seg_lo, LinkRec *d_links,
               uint64_t *owner_counts) {
    hipStream_t st = s->stream;
    const unsigned B = 256;
    drop_step_state(s);  // (held place records' index, and chains ranked on the links this join rewrites)
    constexpr int BT_CS = 14, BT_MAX = 22;  // counting sort's LDS histogram limit; radix sort past it
    EC_CHECK(s->jseg.ensure(((size_t)nowners + 2) * 8 + ((size_t)(1u << BT_MAX) + 1) * 8 + 64));
    unsigned long long *dseg = s->jseg.as<unsigned long long>();
    unsigned long long *bstart = dseg + nowners + 2;
    EC_HIP(hipMemcpyAsync(dseg, seg_lo, ((size_t)nowners + 1) * 8, hipMemcpyHostToDevice, st));
    EC_CHECK(s->jcnt.ensure(16));
    unsigned int *flag = s->jcnt.as<unsigned int>(), *nout = flag + 1;
    EC_CHECK(s->jout.ensure(std::max<uint64_t>(n, 1) * sizeof(LinkRec)));
    LinkRec *outbox = s->jout.as<LinkRec>();
    // join buckets: ~n / 2 junction groups, <= ~900 a 2048-slot table; up to 2^14 buckets by the
    // counting sort (its LDS histogram's limit), up to 2^22 by a radix sort of the bucket ids --
    // sub-buckets (each re-reading its bucket's records) only past that or when forced: config 5's
    // per-rank step joined 4e8 records in 2^14 buckets x 16 sub-buckets in 195 ms.  A table that
    // overflows (skewed junction hashes) retries with 4096 slots, then finer buckets, then more
    // sub-buckets (EULERHIP_JUNCTION_BT / _SB / _CLAIM force the split / a smaller claim cap)
    const int btmax = kn().junction_bt >= 0 ? std::min(kn().junction_bt, BT_MAX) : BT_MAX;
    const double groups = (double)n / 2.0;
    int bt = 0, sb = 0;
    while (bt < btmax && groups / (double)(1ull << bt) > 900.0) bt++;
    while (sb < 8 && groups / (double)(1ull << (bt + sb)) > 900.0) sb++;
    if (kn().junction_sb > sb) sb = std::min(kn().junction_sb, 8);
    bool big = groups / (double)(1ull << (bt + sb)) > 1500.0;
    for (;;) {
        const unsigned int nb = 1u << bt;
        const unsigned int claim = kn().junction_claim > 0 ? (unsigned int)kn().junction_claim
                                                           : (big ? 4096u : 2048u) - 1u;
        EC_CHECK(s->joid.ensure(std::max<uint64_t>(n, 1) * 4));
        EC_HIP(hipMemsetAsync(flag, 0, 8, st));
        if (n) k_junction_bucket<R><<<grid_for(n, B), B, 0, st>>>(d_recs, n, bt, s->joid.as<unsigned int>());
        if ((bt <= BT_CS && kn().junction_radix != 1) || !n) {
            EC_CHECK(bin_sort(s, s->joid.as<unsigned int>(), n, nb, bstart));
        } else {  // record order by bucket id: rocprim radix sort of (id, index) pairs over bt bits
            EC_CHECK(s->mbid.ensure(n * 4));
            EC_CHECK(s->mbid2.ensure(n * 4));
            EC_CHECK(s->midx2.ensure(n * 4));
            k_iota_u32<<<grid_for(n, B, 8192), B, 0, st>>>(s->mbid.as<unsigned int>(), n);
            size_t bytes = 0;
            EC_HIP(rocprim::radix_sort_pairs(nullptr, bytes, s->joid.as<unsigned int>(), s->mbid2.as<unsigned int>(),
                                             s->mbid.as<unsigned int>(), s->midx2.as<unsigned int>(), (size_t)n, 0, bt,
                                             st));
            EC_CHECK(s->tmp.ensure(bytes));
            EC_HIP(rocprim::radix_sort_pairs(s->tmp.p, bytes, s->joid.as<unsigned int>(), s->mbid2.as<unsigned int>(),
                                             s->mbid.as<unsigned int>(), s->midx2.as<unsigned int>(), (size_t)n, 0, bt,
                                             st));
            k_sorted_starts<<<grid_for(n, B, 8192), B, 0, st>>>(s->mbid2.as<unsigned int>(), n, nb, bstart);
        }
        const unsigned int n0 = (unsigned int)(2 * s->seg_lo), n1 = (unsigned int)(2 * (s->seg_lo + s->seg_Ur));
        if (n) {
            if (big)
                k_junction_join<4096, 512, R><<<nb, 512, 0, st>>>(d_recs, s->midx2.as<unsigned int>(), bstart, n0, n1,
                                                                  s->succ.as<unsigned int>(), outbox, nout,
                                                                  (unsigned int)n, flag, bt, sb, claim);
            else
                k_junction_join<2048, 512, R><<<nb, 512, 0, st>>>(d_recs, s->midx2.as<unsigned int>(), bstart, n0, n1,
                                                                  s->succ.as<unsigned int>(), outbox, nout,
                                                                  (unsigned int)n, flag, bt, sb, claim);
            EC_HIP(hipGetLastError());
        }
        // outbox -> destination-major link records, sized by n on the host (the count stays on
        // the device: one read-back for the flags and the destinations' counts)
        if (n) {
            k_link_dest<<<grid_for(n, B), B, 0, st>>>(outbox, nout, (unsigned int)n, dseg, (unsigned int)nowners,
                                                      s->joid.as<unsigned int>());
            EC_CHECK(bin_sort(s, s->joid.as<unsigned int>(), n, (unsigned int)nowners + 1, bstart));
            k_gather_recs<LinkRec><<<grid_for(n, B), B, 0, st>>>(outbox, s->midx2.as<unsigned int>(), n, d_links);
        } else {
            EC_HIP(hipMemsetAsync(bstart, 0, ((size_t)nowners + 2) * 8, st));
        }
        unsigned int hf[2] = {0, 0};
        std::vector<unsigned long long> hs((size_t)nowners + 2);
        EC_CHECK(d2h(s, hf, flag, 8, st));
        EC_CHECK(d2h(s, hs.data(), bstart, ((size_t)nowners + 2) * 8, st));
        EC_CHECK(host_sync(s, st));
        if (hf[0] & 2u) {
            set_error("junction join: link outbox overflow");
            return EC_ERR_STATE;
        }
        if (hf[0] & 1u) {  // a table past its slots: bigger tables, finer buckets, more sub-buckets
            // (succ: a failed attempt's local links are the same links the retry writes)
            if (!big) big = true;
            else if (bt < btmax) bt++;
            else if (sb < 8) sb++;
            else {
                set_error("junction join: a bucket of %llu records overflows its table at 2^%d x 2^%d buckets",
                          (unsigned long long)n, bt, sb);
                return EC_ERR_CAPACITY;
            }
            s->stats.table_retries++;
            continue;
        }
        for (int r = 0; r < nowners; r++) owner_counts[r] = hs[r + 1] - hs[r];
        return EC_OK;
    }
}

extern "C" {

int ec_graph_place(ec_session *s, uint64_t lo, uint64_t U, int nowners, void *d_jrecs, uint64_t *owner_counts,
                   uint64_t *n_pal) {
    refresh_knobs();
    if (!s || nowners < 1 || nowners > MAX_OWNERS || !owner_counts || !n_pal || lo + s->n_dense > U ||
        2 * U >= (uint64_t)CYC) {
        set_error("ec_graph_place: bad arguments (segment [%llu, +%u) of %llu ids)", (unsigned long long)lo,
                  s ? s->n_dense : 0u, (unsigned long long)U);
        return EC_ERR_ARG;
    }
    EC_HIP(hipSetDevice(s->device));
    return s->k > 32 ? graph_place<K128>(s, lo, U, nowners, d_jrecs, owner_counts, n_pal)
                     : graph_place<unsigned long long>(s, lo, U, nowners, d_jrecs, owner_counts, n_pal);
}

int ec_graph_join(ec_session *s, const void *d_jrecs, uint64_t n, int nowners, const uint64_t *seg_lo, void *d_links,
                  uint64_t *owner_counts) {
    if (!s || !s->placed || nowners < 1 || nowners > MAX_OWNERS || !seg_lo || !owner_counts ||
        (n && (!d_jrecs || !d_links))) {
        set_error("ec_graph_join: no placed segment or bad arguments");
        return EC_ERR_ARG;
    }
    for (int r = 0; r < nowners; r++)
        if (seg_lo[r] > seg_lo[r + 1] || seg_lo[nowners] != s->n_dense) {
            set_error("ec_graph_join: segment bounds not ascending up to %u", s->n_dense);
            return EC_ERR_ARG;
        }
    EC_HIP(hipSetDevice(s->device));
    return s->k > 32 ? graph_join<RecJ>(s, static_cast<const RecJ *>(d_jrecs), n, nowners, seg_lo,
                                        static_cast<LinkRec *>(d_links), owner_counts)
                     : graph_join<RecJ64>(s, static_cast<const RecJ64 *>(d_jrecs), n, nowners, seg_lo,
                                          static_cast<LinkRec *>(d_links), owner_counts);
}

int ec_graph_links_apply(ec_session *s, const void *d_links, uint64_t n) {
    if (!s || !s->placed || (n && !d_links)) {
        set_error("ec_graph_links_apply: no placed segment");
        return EC_ERR_ARG;
    }
    drop_step_state(s);  // (the links change: chains ranked on them are stale)
    EC_HIP(hipSetDevice(s->device));
    hipStream_t st = s->stream;
    EC_CHECK(s->jcnt.ensure(16));
    unsigned int *bad = s->jcnt.as<unsigned int>();
    EC_HIP(hipMemsetAsync(bad, 0, 4, st));
    if (n)
        k_links_apply<<<grid_for(n, 256), 256, 0, st>>>(static_cast<const LinkRec *>(d_links), n,
                                                        (unsigned int)(2 * s->seg_lo),
                                                        (unsigned int)(2 * (s->seg_lo + s->seg_Ur)),
                                                        s->succ.as<unsigned int>(), bad);
    unsigned int hb = 0;
    EC_CHECK(d2h(s, &hb, bad, 4, st));
    EC_CHECK(host_sync(s, st));
    if (hb) {
        set_error("ec_graph_links_apply: a link record names a node outside this segment");
        return EC_ERR_ARG;
    }
    return EC_OK;
}

int ec_super_record_bytes(void) { return (int)sizeof(SuperRec); }
int ec_start_record_bytes(void) { return (int)sizeof(StartRec); }

int ec_assemble_from_kmers(ec_session *s, const char *kmers, const uint32_t *counts, uint64_t n, int k, unsigned flags) {
    if (!s || (n && (!kmers || !counts))) {
        set_error("null argument");
        return EC_ERR_ARG;
    }
    EC_CHECK(begin_call(s, k, flags));
    hipStream_t st = s->stream;
    EC_CHECK(s->dchars.ensure(std::max<size_t>(n * (size_t)k, 1)));
    EC_CHECK(s->dcounts.ensure(std::max<size_t>(n * 4, 4)));
    const bool wide = k > 32;
    EC_CHECK(s->recs2.ensure(std::max<size_t>(n * (wide ? sizeof(AggW) : sizeof(Agg)), 16)));
    Scalars *dsc = s->scal.as<Scalars>();
    if (n) {
        EC_HIP(hipMemcpyAsync(s->dchars.p, kmers, n * (size_t)k, hipMemcpyHostToDevice, st));
        EC_HIP(hipMemcpyAsync(s->dcounts.p, counts, n * 4, hipMemcpyHostToDevice, st));
        if (wide)
            k_kmers_to_agg<OpsW><<<grid_for(n, 256), 256, 0, st>>>(s->dchars.as<char>(), s->dcounts.as<unsigned int>(),
                                                                  n, k, s->recs2.as<AggW>(), &dsc->bad);
        else
            k_kmers_to_agg<Ops64><<<grid_for(n, 256), 256, 0, st>>>(s->dchars.as<char>(), s->dcounts.as<unsigned int>(),
                                                                   n, k, s->recs2.as<Agg>(), &dsc->bad);
        unsigned long long bad = 0;
        EC_CHECK(d2h(s, &bad, &dsc->bad, 8, st));
        EC_CHECK(host_sync(s, st));
        if (bad != ~0ull)  // bytes other than A/C/G/T: opaque symbols (extended.h)
            return assemble_kmers_extended(s, kmers, n, k);
    }
    unsigned int U = 0;
    if (wide) {
        SolidIndexW sidx{};
        EC_CHECK(phase_merge_w(s, s->recs2.as<AggW>(), n, LLONG_MIN, U, sidx));
        return phase_graph<OpsW>(s, k, U, sidx);
    }
    SolidIndex sidx{};
    EC_CHECK(phase_merge(s, s->recs2.as<Agg>(), n, LLONG_MIN, U, sidx));
    return phase_graph<Ops64>(s, k, U, sidx);
}

}  // extern "C"

// ---- tip clipping (clip.h) ---------------------------------------------------------------------
namespace {

// the rule on the session's current results: the clipped contigs into clip_list, their count and
// k-mer windows into tot (the round's only read-back)
int clip_evaluate(ec_session *s, unsigned int nc, unsigned long long max_len, ClipTotals &tot) {
    hipStream_t st = s->stream;
    tot = ClipTotals{};
    if (!nc) return EC_OK;
    EC_CHECK(s->clip_cand.ensure(nc));
    EC_CHECK(s->clip_list.ensure((size_t)nc * 4));
    EC_CHECK(s->clip_tot.ensure(sizeof(ClipTotals)));
    EC_HIP(hipMemsetAsync(s->clip_tot.p, 0, sizeof(ClipTotals), st));
    k_clip_cand<<<grid_for(nc, 256), 256, 0, st>>>(s->coff.as<unsigned long long>(), s->lcnt.as<unsigned int>(), nc,
                                                   max_len, s->clip_cand.as<uint8_t>());
    k_clip_pick<<<grid_for(nc, 256), 256, 0, st>>>(s->coff.as<unsigned long long>(), s->lk.as<long long>(),
                                                   s->lcnt.as<unsigned int>(), s->clip_cand.as<uint8_t>(), nc, s->k,
                                                   s->clip_list.as<unsigned int>(), s->clip_tot.as<ClipTotals>());
    EC_CHECK(d2h(s, &tot, s->clip_tot.p, sizeof(ClipTotals), st));
    return host_sync(s, st);
}

// the back half of a round, shared by the clean-ups and ec_refilter: the dense arrays exported with
// the ids marked in clip_kill as fillers into recs2 (as ec_assemble_from_kmers holds its records),
// then the merge and the graph phase of ec_assemble_from_solid on them.  recs2 is no scratch of the
// merge or the graph phase, and nothing else crosses the round.
template <typename Ops, typename Index>
int regraph_round(ec_session *s, unsigned int U) {
    using K = typename Ops::K;
    using Rec = typename RecOf<K>::T;
    hipStream_t st = s->stream;
    const int k = s->k;
    EC_CHECK(s->recs2.ensure(std::max<size_t>((size_t)U * sizeof(Rec), 16)));
    k_clip_export<K><<<grid_for(U, 256), 256, 0, st>>>(s->dkey.as<K>(), s->dcnt.as<unsigned int>(),
                                                       s->dfc.as<unsigned long long>(),
                                                       s->dft.as<unsigned long long>(), s->clip_kill.as<uint8_t>(), U,
                                                       s->recs2.as<Rec>());
    // from here the call starts from inputs: the counting fields of the stats stay the assembly's
    const ec_stats was = s->stats;
    const unsigned flags = s->flags & ~(EC_FLAG_TIMING | EC_FLAG_KERNEL_TIMING);
    EC_CHECK(begin_call(s, k, flags));
    unsigned int U2 = 0;
    Index sidx{};
    if constexpr (std::is_same<Index, SolidIndexW>::value)
        EC_CHECK(phase_merge_w(s, s->recs2.as<AggW>(), U, LLONG_MIN, U2, sidx));
    else
        EC_CHECK(phase_merge(s, s->recs2.as<Agg>(), U, LLONG_MIN, U2, sidx));
    EC_CHECK((phase_graph<Ops, Index>(s, k, U2, sidx)));
    ec_stats &now = s->stats;
    now.n_reads = was.n_reads;
    now.n_positions = was.n_positions;
    now.n_distinct_est = was.n_distinct_est;
    now.n_distinct = was.n_distinct;
    now.table_capacity = was.table_capacity;
    now.table_retries = was.table_retries;
    now.n_records = was.n_records;
    now.count_path = was.count_path;
    now.count_variant = was.count_variant;
    now.n_buckets = was.n_buckets;
    now.record_bytes = was.record_bytes;
    return EC_OK;
}

// one clipping round: the listed contigs' k-mers marked (the index is read before the merge
// rewrites it), then the back half
template <typename Ops, typename Index>
int clip_round(ec_session *s, const Index &idx, unsigned int n_clip, unsigned int U) {
    hipStream_t st = s->stream;
    EC_CHECK(s->clip_kill.ensure(std::max<size_t>(U, 1)));
    EC_HIP(hipMemsetAsync(s->clip_kill.p, 0, std::max<size_t>(U, 1), st));
    k_clip_kill<Ops, Index><<<grid_for((uint64_t)n_clip * 64, 256), 256, 0, st>>>(
        idx, s->clip_list.as<unsigned int>(), n_clip, s->coff.as<unsigned long long>(), s->chars.as<char>(), s->k, U,
        s->clip_kill.as<uint8_t>());
    return regraph_round<Ops, Index>(s, U);
}

// ---- bubble popping, per-contig k-mer count sums (pop.h) ----------------------------------------
// S_i of the contigs (sel: only of those whose sel[i] is not POP_NONE) into pop_sum, on the stream
template <typename Ops, typename Index>
int ksum_run(ec_session *s, const Index &idx, unsigned int nc, const unsigned long long *sel) {
    hipStream_t st = s->stream;
    const unsigned int U = (unsigned int)s->stats.n_solid;
    // every contig has at most ceil(W / KSUM_TILE) <= 1 + chars / KSUM_TILE tiles
    const unsigned long long cap = (unsigned long long)nc + s->stats.n_contig_chars / KSUM_TILE + 1;
    if (cap >= (1ull << 32)) {
        set_error("contig k-mer sums: %llu tiles at most, >= 2^32", cap);
        return EC_ERR_CAPACITY;
    }
    EC_CHECK(s->pop_sum.ensure((size_t)nc * 8));
    EC_CHECK(s->pop_tcnt.ensure((size_t)nc * 4));
    EC_CHECK(s->pop_toff.ensure((size_t)nc * 4));
    EC_CHECK(s->pop_tile.ensure((size_t)cap * 4));
    EC_HIP(hipMemsetAsync(s->pop_sum.p, 0, (size_t)nc * 8, st));
    EC_HIP(hipMemsetAsync(s->pop_tile.p, 0xFF, (size_t)cap * 4, st));  // (no contig: the tile is skipped)
    k_ksum_count<<<grid_for(nc, 256), 256, 0, st>>>(s->coff.as<unsigned long long>(), nc, s->k, sel,
                                                    s->pop_tcnt.as<unsigned int>());
    EC_CHECK(scan_excl_u32(s, s->pop_tcnt.as<unsigned int>(), s->pop_toff.as<unsigned int>(), nc));
    k_ksum_tiles<<<grid_for((uint64_t)nc * 64, 256), 256, 0, st>>>(s->pop_tcnt.as<unsigned int>(),
                                                                   s->pop_toff.as<unsigned int>(), nc,
                                                                   (unsigned int)cap, s->pop_tile.as<unsigned int>());
    k_contig_ksum<Ops, Index><<<(unsigned int)((cap + 3) / 4), 256, 0, st>>>(
        idx, s->pop_tile.as<unsigned int>(), s->pop_toff.as<unsigned int>(), (unsigned int)cap, nc,
        s->coff.as<unsigned long long>(), s->chars.as<char>(), s->dcnt.as<unsigned int>(), s->k, U,
        s->pop_sum.as<unsigned long long>());
    EC_HIP(hipGetLastError());
    return EC_OK;
}

int ksum_any(ec_session *s, unsigned int nc, const unsigned long long *sel) {
    if (s->k > 32) return ksum_run<OpsW, SolidIndexW>(s, s->cidxw, nc, sel);
    return ksum_run<Ops64, SolidIndex>(s, s->cidx, nc, sel);
}

// the bubble rule on the session's current results, as clip_evaluate: popped contigs into clip_list
int pop_evaluate(ec_session *s, unsigned int nc, unsigned long long max_len, ClipTotals &tot) {
    hipStream_t st = s->stream;
    tot = ClipTotals{};
    if (!nc) return EC_OK;
    EC_CHECK(s->pop_key.ensure((size_t)nc * 8));
    EC_CHECK(s->clip_list.ensure((size_t)nc * 4));
    EC_CHECK(s->clip_tot.ensure(sizeof(ClipTotals)));
    EC_HIP(hipMemsetAsync(s->clip_tot.p, 0, sizeof(ClipTotals), st));
    k_pop_cand<<<grid_for(nc, 256), 256, 0, st>>>(s->coff.as<unsigned long long>(), s->lk.as<long long>(),
                                                  s->lcnt.as<unsigned int>(), nc, max_len,
                                                  s->pop_key.as<unsigned long long>());
    EC_CHECK(ksum_any(s, nc, s->pop_key.as<unsigned long long>()));
    k_pop_pick<<<grid_for(nc, 256), 256, 0, st>>>(s->coff.as<unsigned long long>(), s->lk.as<long long>(),
                                                  s->lcnt.as<unsigned int>(), s->pop_key.as<unsigned long long>(),
                                                  s->pop_sum.as<unsigned long long>(), nc, s->k,
                                                  s->clip_list.as<unsigned int>(), s->clip_tot.as<ClipTotals>());
    EC_CHECK(d2h(s, &tot, s->clip_tot.p, sizeof(ClipTotals), st));
    return host_sync(s, st);
}

// the loop of ec_clip_tips and ec_pop_bubbles: evaluate the rule, stop if it lists nothing, else
// remove the listed contigs' k-mers and run the graph phase again (clip_round)
template <typename Eval>
int cleanup_loop(ec_session *s, uint32_t max_rounds, Eval eval, uint32_t &rounds, uint32_t &converged,
                 uint64_t &n_contigs, uint64_t &n_kmers) {
    EC_HIP(hipSetDevice(s->device));
    drop_step_state(s);
    s->dense_ok = false;
    for (uint32_t r = 0; r < max_rounds; r++) {
        ClipTotals tot{};
        EC_CHECK(eval((unsigned int)s->stats.n_contigs, tot));
        if (!tot.n_clip) {
            converged = 1;
            break;
        }
        const unsigned int U = (unsigned int)s->stats.n_solid;
        if (s->k > 32) EC_CHECK((clip_round<OpsW, SolidIndexW>(s, s->cidxw, tot.n_clip, U)));
        else EC_CHECK((clip_round<Ops64, SolidIndex>(s, s->cidx, tot.n_clip, U)));
        rounds++;
        n_contigs += tot.n_clip;
        n_kmers += tot.n_kmer;
    }
    return EC_OK;
}

// the refusals ec_clip_tips, ec_pop_bubbles, ec_copy_contig_kmer_sums, ec_kmer_spectrum and
// ec_refilter share
int clip_state_check(ec_session *s, const char *who) {
    if (s->clip_ok) return EC_OK;
    set_error("%s needs the device state of a one-GPU assembly (ec_assemble_*, _from_solid, _from_kmers, "
              "ec_clip_tips, ec_pop_bubbles, ec_refilter): %s", who, s->clip_why);
    return EC_ERR_STATE;
}

}  // namespace

extern "C" int ec_clip_tips(ec_session *s, uint32_t max_tip_len, uint32_t max_rounds, ec_clip_info *info) {
    if (!s || !info) {
        set_error("ec_clip_tips: null session / info");
        return EC_ERR_ARG;
    }
    if (max_rounds == 0) {
        set_error("ec_clip_tips: max_rounds = 0");
        return EC_ERR_ARG;
    }
    EC_CHECK(clip_state_check(s, "ec_clip_tips"));
    *info = ec_clip_info{};
    const unsigned long long max_len = max_tip_len ? max_tip_len : 2ull * (unsigned)s->k;
    return cleanup_loop(
        s, max_rounds, [&](unsigned int nc, ClipTotals &tot) { return clip_evaluate(s, nc, max_len, tot); },
        info->rounds, info->converged, info->n_tip_contigs, info->n_tip_kmers);
}

extern "C" int ec_pop_bubbles(ec_session *s, uint32_t max_bubble_len, uint32_t max_rounds, ec_pop_info *info) {
    if (max_bubble_len > 65535) {
        set_error("ec_pop_bubbles: max_bubble_len %u > 65535", max_bubble_len);
        return EC_ERR_ARG;
    }
    if (!s || !info) {
        set_error("ec_pop_bubbles: null session / info");
        return EC_ERR_ARG;
    }
    if (max_rounds == 0) {
        set_error("ec_pop_bubbles: max_rounds = 0");
        return EC_ERR_ARG;
    }
    EC_CHECK(clip_state_check(s, "ec_pop_bubbles"));
    *info = ec_pop_info{};
    const unsigned long long max_len = max_bubble_len ? max_bubble_len : 2ull * (unsigned)s->k;
    return cleanup_loop(
        s, max_rounds, [&](unsigned int nc, ClipTotals &tot) { return pop_evaluate(s, nc, max_len, tot); },
        info->rounds, info->converged, info->n_bubble_contigs, info->n_bubble_kmers);
}

extern "C" int ec_copy_contig_kmer_sums(ec_session *s, uint64_t *sums) {
    if (!s || !sums) {
        set_error("ec_copy_contig_kmer_sums: null session / sums");
        return EC_ERR_ARG;
    }
    EC_CHECK(clip_state_check(s, "ec_copy_contig_kmer_sums"));
    const unsigned int nc = (unsigned int)s->stats.n_contigs;
    if (!nc) return EC_OK;
    EC_HIP(hipSetDevice(s->device));
    EC_CHECK(ksum_any(s, nc, nullptr));
    EC_CHECK(d2h(s, sums, s->pop_sum.p, (size_t)nc * 8, s->stream));
    return host_sync(s, s->stream);
}

// ---- k-mer count spectrum, re-filter by a new solid limit (spectrum.h) -------------------------
extern "C" int ec_kmer_spectrum(ec_session *s, uint32_t nbins, uint64_t *hist) {
    if (nbins < 2 || nbins > EC_SPECTRUM_MAX_BINS) {
        set_error("ec_kmer_spectrum: nbins %u outside [2, %d]", nbins, EC_SPECTRUM_MAX_BINS);
        return EC_ERR_ARG;
    }
    if (!s || !hist) {
        set_error("ec_kmer_spectrum: null session / hist");
        return EC_ERR_ARG;
    }
    EC_CHECK(clip_state_check(s, "ec_kmer_spectrum"));
    std::memset(hist, 0, (size_t)nbins * 8);
    const unsigned int U = (unsigned int)s->stats.n_solid;
    if (!U) return EC_OK;
    EC_HIP(hipSetDevice(s->device));
    hipStream_t st = s->stream;
    EC_CHECK(s->spec_hist.ensure((size_t)nbins * 8));
    EC_HIP(hipMemsetAsync(s->spec_hist.p, 0, (size_t)nbins * 8, st));
    k_spectrum<<<grid_for((U + 3ull) / 4, 256, 2048), 256, 0, st>>>(s->dcnt.as<unsigned int>(), U, nbins,
                                                                   s->spec_hist.as<unsigned long long>());
    EC_HIP(hipGetLastError());
    EC_CHECK(d2h(s, hist, s->spec_hist.p, (size_t)nbins * 8, st));
    return host_sync(s, st);
}

extern "C" int ec_refilter(ec_session *s, uint32_t limit, ec_refilter_info *info) {
    if (!s || !info) {
        set_error("ec_refilter: null session / info");
        return EC_ERR_ARG;
    }
    EC_CHECK(clip_state_check(s, "ec_refilter"));
    *info = ec_refilter_info{};
    info->limit = limit;
    EC_HIP(hipSetDevice(s->device));
    drop_step_state(s);
    s->dense_ok = false;
    const unsigned int U = (unsigned int)s->stats.n_solid;
    if (!U) return EC_OK;
    hipStream_t st = s->stream;
    RefilterTotals tot{};
    EC_CHECK(s->clip_kill.ensure(U));
    EC_CHECK(s->clip_tot.ensure(sizeof(RefilterTotals)));
    EC_HIP(hipMemsetAsync(s->clip_tot.p, 0, sizeof(RefilterTotals), st));
    k_refilter_mark<<<grid_for((U + 3ull) / 4, 256, 2048), 256, 0, st>>>(
        s->dcnt.as<unsigned int>(), U, limit, s->clip_kill.as<uint8_t>(), s->clip_tot.as<RefilterTotals>());
    EC_HIP(hipGetLastError());
    EC_CHECK(d2h(s, &tot, s->clip_tot.p, sizeof(RefilterTotals), st));
    EC_CHECK(host_sync(s, st));
    if (!tot.n_removed) return EC_OK;  // (nothing at or below the limit: every result byte stays)
    if (s->k > 32) EC_CHECK((regraph_round<OpsW, SolidIndexW>(s, U)));
    else EC_CHECK((regraph_round<Ops64, SolidIndex>(s, U)));
    info->changed = 1;
    info->n_removed_kmers = tot.n_removed;
    return EC_OK;
}

// ---- the same on the held dense records of the sharded path (dense_filter.h) --------------------
static int dense_state_check(ec_session *s, const char *who) {
    if (s->dense_ok) return EC_OK;
    set_error("%s: no counted or merged records (ec_count_shard / ec_merge_owned*), or a later call replaced them", who);
    return EC_ERR_STATE;
}

extern "C" int ec_dense_spectrum(ec_session *s, uint32_t nbins, uint64_t *hist) {
    if (nbins < 2 || nbins > EC_SPECTRUM_MAX_BINS) {
        set_error("ec_dense_spectrum: nbins %u outside [2, %d]", nbins, EC_SPECTRUM_MAX_BINS);
        return EC_ERR_ARG;
    }
    if (!s || !hist) {
        set_error("ec_dense_spectrum: null session / hist");
        return EC_ERR_ARG;
    }
    EC_CHECK(dense_state_check(s, "ec_dense_spectrum"));
    std::memset(hist, 0, (size_t)nbins * 8);
    const unsigned int n = s->n_dense;
    if (!n) return EC_OK;
    EC_HIP(hipSetDevice(s->device));
    hipStream_t st = s->stream;
    EC_CHECK(s->spec_hist.ensure((size_t)nbins * 8));
    EC_HIP(hipMemsetAsync(s->spec_hist.p, 0, (size_t)nbins * 8, st));
    k_spectrum<<<grid_for((n + 3ull) / 4, 256, 2048), 256, 0, st>>>(s->dcnt.as<unsigned int>(), n, nbins,
                                                                   s->spec_hist.as<unsigned long long>());
    EC_HIP(hipGetLastError());
    EC_CHECK(d2h(s, hist, s->spec_hist.p, (size_t)nbins * 8, st));
    return host_sync(s, st);
}

template <typename K>
static int dense_compact(ec_session *s, unsigned int n, unsigned int kept, unsigned int nblk, unsigned int limit) {
    hipStream_t st = s->stream;
    // (scratch first: a failed allocation leaves the held records as they are)
    EC_CHECK(s->recs.ensure((size_t)n * sizeof(K)));
    EC_CHECK(s->midx.ensure((size_t)n * 4));
    EC_CHECK(s->recs2.ensure((size_t)n * 16));
    unsigned int *bc = s->rbc.as<unsigned int>(), *bs = bc + nblk;
    unsigned long long *ofc = s->recs2.as<unsigned long long>(), *oft = ofc + n;
    EC_CHECK(scan_incl_u32(s, bc, bs, nblk));
    k_dense_write<K><<<nblk, 256, 0, st>>>(s->dkey.as<K>(), s->dcnt.as<unsigned int>(), s->dfc.as<unsigned long long>(),
                                          s->dft.as<unsigned long long>(), n, limit, bs, s->recs.as<K>(),
                                          s->midx.as<unsigned int>(), ofc, oft);
    EC_HIP(hipGetLastError());
    if (kept) {
        EC_HIP(hipMemcpyAsync(s->dkey.p, s->recs.p, (size_t)kept * sizeof(K), hipMemcpyDeviceToDevice, st));
        EC_HIP(hipMemcpyAsync(s->dcnt.p, s->midx.p, (size_t)kept * 4, hipMemcpyDeviceToDevice, st));
        EC_HIP(hipMemcpyAsync(s->dfc.p, ofc, (size_t)kept * 8, hipMemcpyDeviceToDevice, st));
        EC_HIP(hipMemcpyAsync(s->dft.p, oft, (size_t)kept * 8, hipMemcpyDeviceToDevice, st));
    }
    return EC_OK;
}

extern "C" int ec_dense_refilter(ec_session *s, uint32_t limit, ec_refilter_info *info) {
    if (!s || !info) {
        set_error("ec_dense_refilter: null session / info");
        return EC_ERR_ARG;
    }
    EC_CHECK(dense_state_check(s, "ec_dense_refilter"));
    *info = ec_refilter_info{};
    info->limit = limit;
    const unsigned int n = s->n_dense;
    if (!n) return EC_OK;
    EC_HIP(hipSetDevice(s->device));
    hipStream_t st = s->stream;
    const unsigned int nblk = (unsigned int)((n + (uint64_t)DF_SPAN - 1) / DF_SPAN);
    RefilterTotals tot{};
    EC_CHECK(s->rbc.ensure((size_t)nblk * 8));
    EC_CHECK(s->clip_tot.ensure(sizeof(RefilterTotals)));
    EC_HIP(hipMemsetAsync(s->clip_tot.p, 0, sizeof(RefilterTotals), st));
    k_dense_count<<<nblk, 256, 0, st>>>(s->dcnt.as<unsigned int>(), n, limit, s->rbc.as<unsigned int>(),
                                        s->clip_tot.as<RefilterTotals>());
    EC_HIP(hipGetLastError());
    EC_CHECK(d2h(s, &tot, s->clip_tot.p, sizeof(RefilterTotals), st));
    EC_CHECK(host_sync(s, st));
    if (!tot.n_removed) return EC_OK;  // (nothing at or below the limit: every held byte stays)
    const unsigned int kept = n - (unsigned int)tot.n_removed;
    if (s->k > 32) EC_CHECK(dense_compact<K128>(s, n, kept, nblk, limit));
    else EC_CHECK(dense_compact<unsigned long long>(s, n, kept, nblk, limit));
    // what was derived from the old set: pending step records, the cached owner ids of a counts-only
    // ec_export_by_owner, the merge's bucket marks (they cut the old ids)
    drop_step_state(s);
    s->own_valid = false;
    s->bmark_ok = false;
    s->seg_marks = 0;
    s->n_dense = kept;
    s->stats.n_solid = kept;
    info->changed = 1;
    info->n_removed_kmers = tot.n_removed;
    return EC_OK;
}
