// count_phase.h -- the host side of the count phases: from the reads (or exchanged records) to the
// dense solid arrays and their lookup index, for both key widths.
//   k <= 32: phase_count -> phase_count_v2 -> phase_count_sk2 (super-k-mer records, count_sk2.h),
//            window records (count_v2.h), the exact path (count_part.h), the HBM table
//   k > 32:  phase_count_w -> phase_count_wpart (count_wide.h)
//   merges / loads of the sharded path: phase_merge_part, phase_merge, phase_merge_w,
//            phase_load_det, phase_load_det_w
// One header in the one translation unit, like session.h, which it stands on together with the
// kernel headers.  The graph phase's links prologue that phase_count_sk2 queues behind its bucket
// kernel lives with links_local in assemble.hip (declared below).
#pragma once
#include "common.h"
#include "compact.h"
#include "count_global.h"
#include "count_part.h"
#include "count_sk2.h"
#include "count_v2.h"
#include "count_wide.h"
#include "extended.h"
#include "graph.h"
#include "hostin.h"
#include "shard.h"
#include "session.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace {

// what launch_bucket needs besides the records and the table size
struct BucketArgs {
    // bucket b = records [bbeg[b], bend[b]): the fixed-capacity buckets of count_v2.h; null =
    // the exact path's scanned starts (s->bstart)
    const unsigned long long *bbeg = nullptr, *bend = nullptr;
    bool filt = false;             // k_bucket_filt (more distinct keys than LDS tables hold)
    int pmin = 0, pmax = 1;        // ... with 2^pmin .. 2^pmax part tables per bucket region
    unsigned int *bmark = nullptr; // k_bucket: one bit per dense id, set at each bucket's first
};
// the seen-twice filter's fields of a BucketPlan (EULERHIP_FILTER_PMIN: at least 2^pmin part tables)
BucketArgs filter_args(bool filt, int pmax) {
    BucketArgs a;
    a.filt = filt;
    a.pmax = pmax;
    a.pmin = kn().filter_pmin >= 0 ? std::max(0, std::min(pmax, kn().filter_pmin)) : 0;
    return a;
}

template <typename Src>
int launch_bucket(ec_session *s, Src src, unsigned nb, unsigned slots, long long limit, BucketArgs a = {}) {
    Scalars *dsc = s->scal.as<Scalars>();
    hipStream_t st = s->stream;
    const unsigned long long *bb = a.bbeg ? a.bbeg : s->bstart.as<unsigned long long>();
    const unsigned long long *be = a.bbeg ? a.bend : s->bstart.as<unsigned long long>() + 1;
    if (a.filt) {  // error-rich input: seen-twice filter + two half tables per bucket
        EC_CHECK(s->bnp.ensure(nb));
        k_bucket_filt<Src><<<nb, BUCKET_THREADS, 0, st>>>(
            src, bb, be, 1u, limit, a.pmin, a.pmax, (float)PART_KEYS,
            s->dkey.as<unsigned long long>(),
            s->dcnt.as<unsigned int>(), s->dfc.as<unsigned long long>(), s->dft.as<unsigned long long>(),
            s->no_index ? nullptr : s->sub.as<SubSlot>(), s->bnp.as<uint8_t>(), &dsc->nsolid, &dsc->ndistinct,
            &dsc->overflow);
        return EC_OK;
    }
    if (slots == 2048)
        k_bucket<Src, 2048><<<nb, BUCKET_THREADS, 0, st>>>(
            src, bb, be, 1u, limit, s->dkey.as<unsigned long long>(), s->dcnt.as<unsigned int>(),
            s->dfc.as<unsigned long long>(), s->dft.as<unsigned long long>(), s->no_index ? nullptr : s->sub.as<SubSlot>(), &dsc->nsolid,
            &dsc->ndistinct, &dsc->overflow, a.bmark);
    else
        k_bucket<Src, 4096><<<nb, BUCKET_THREADS, 0, st>>>(
            src, bb, be, 1u, limit, s->dkey.as<unsigned long long>(), s->dcnt.as<unsigned int>(),
            s->dfc.as<unsigned long long>(), s->dft.as<unsigned long long>(), s->no_index ? nullptr : s->sub.as<SubSlot>(), &dsc->nsolid,
            &dsc->ndistinct, &dsc->overflow, a.bmark);
    return EC_OK;
}

// Bucket geometry of the partitioned path from the distinct estimate (shared by count_part.h's
// exact path and count_v2.h): 2^bbits final buckets of <= ~1100 keys, 2048- or 4096-slot LDS
// tables, or k_bucket_filt's seen-twice filter / part tables past ~2400 keys per bucket.
struct BucketPlan {
    bool part = false;  // partitioned counting applies at all (else the HBM table)
    bool filt = false;
    int pmax = 1;
    int bbits = 0;
    unsigned int slots = 2048;
};
BucketPlan plan_buckets(double est, long long limit) {
    constexpr int PMAX = 3;
    BucketPlan p;
    const double filt_max = limit >= 1 ? 32768.0 : PART_KEYS * (1 << PMAX);
    p.part = est / FINE <= 2400.0 || est / FINE <= filt_max;
    p.filt = p.part && (est / FINE > 2400.0 || kn().force_filter);
    while (p.pmax < PMAX && est / FINE / (double)(1 << p.pmax) > PART_KEYS) p.pmax++;
    if (kn().filter_pmax) p.pmax = std::max(1, std::min(PMAX, kn().filter_pmax));
    while (p.bbits < FINE_BITS && est / (double)(1ull << p.bbits) > 1100.0) p.bbits++;
    p.slots = p.filt ? (2048u << p.pmax) : est / (double)(1ull << p.bbits) > 1100.0 ? 4096u : 2048u;
    return p;
}

// ---- count_sk2.h: super-k-mer records for 21 <= k <= 32 -----------------------------------------
// phase_count_sk2 (below) runs these stages in order: sk2_shape, sk2_partition, sk2_refine (on
// speculation, as planned, or again after a bucket overflow), sk2_plan, sk2_buckets,
// sk2_print_stats, and the graph phase's links_prologue behind the bucket kernel.

// Every k_skpart_w<NPF, W, VAL, N17> the library holds, by (npf, w, val, n17): 3 x 12 x 2, plus
// 3 x 2 of the W = 17 form that keeps 17-window runs whole (count_sk2.h sk2_nmax); null: none.
// The one table: the occupancy query (skpart_slots) and the launch (sk2_partition) read it.
// Register-block minima for every window width of 21 <= k <= 32 (w = k - 14; an LDS-ring
// sliding minimum measured 2.19 against 1.60 ms at k = 31).
using SkPartFn = decltype(&k_skpart_w<4, 7, false>);
template <int NPF, bool VAL>
SkPartFn skpart_kernel_w(int w, bool n17) {
    switch (w) {
        case 7: return &k_skpart_w<NPF, 7, VAL>;
        case 8: return &k_skpart_w<NPF, 8, VAL>;
        case 9: return &k_skpart_w<NPF, 9, VAL>;
        case 10: return &k_skpart_w<NPF, 10, VAL>;
        case 11: return &k_skpart_w<NPF, 11, VAL>;
        case 12: return &k_skpart_w<NPF, 12, VAL>;
        case 13: return &k_skpart_w<NPF, 13, VAL>;
        case 14: return &k_skpart_w<NPF, 14, VAL>;
        case 15: return &k_skpart_w<NPF, 15, VAL>;
        case 16: return &k_skpart_w<NPF, 16, VAL>;
        case 17: return n17 ? &k_skpart_w<NPF, 17, VAL, true> : &k_skpart_w<NPF, 17, VAL>;
        case 18: return &k_skpart_w<NPF, 18, VAL>;  // k = 32
    }
    return nullptr;
}
SkPartFn skpart_kernel(int npf, int w, bool val, bool n17) {
    switch (npf) {
        case 4: return val ? skpart_kernel_w<4, true>(w, n17) : skpart_kernel_w<4, false>(w, n17);
        case 7: return val ? skpart_kernel_w<7, true>(w, n17) : skpart_kernel_w<7, false>(w, n17);
        case 10: return val ? skpart_kernel_w<10, true>(w, n17) : skpart_kernel_w<10, false>(w, n17);
    }
    return nullptr;
}

// workgroups of k_skpart_w<npf, w, val> the device runs at once (CUs x resident per CU)
// (n17: the W = 17 form that keeps 17-window runs whole, count_sk2.h sk2_nmax)
static uint64_t skpart_slots(int npf, int w, bool val, bool n17) {
    static thread_local int cache[3][SK_W_MAX + 2][2] = {};
    const int ni = npf == 4 ? 0 : npf == 7 ? 1 : 2;
    int &c = cache[ni][n17 ? SK_W_MAX + 1 : w][val];
    if (!c) {
        const void *fn = (const void *)skpart_kernel(npf, w, val, n17);
        int dev = 0, ncu = 0, per = 0;
        if (!fn || hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, fn, PT_THREADS, 0) != hipSuccess || per < 1)
            return 1;
        c = ncu * per;
    }
    return (uint64_t)c;
}

constexpr uint64_t SK2_C = 1ull << SK2_CBITS;  // coarse buckets of the partition

// one call of phase_count_sk2: its inputs, and the shape sk2_shape derives from them
struct Sk2Call {
    ec_session *s;
    const uint8_t *d_reads;
    const uint64_t *d_off;
    uint64_t nreads, read_base;
    int k;
    long long limit;
    uint32_t M;
    uint64_t P;  // positions (validate: nreads M, until the partition has counted them)
    int npf;
    bool validate;
    // the shape
    bool n17 = false;          // k = 31 on reads of M <= 128 windows: 17-window runs stay whole
    uint64_t G = 0, gsize = 0;  // read groups, reads a group
    uint64_t cap = 0;          // records a (coarse bucket, group) run holds
    uint32_t smask = 0;        // HyperLogLog sample mask
    uint32_t elim = 0;         // entries a partition wave buffers
    MinCfg mc{};
    bool chunked = false;      // (sk2_partition) host input still arriving: one launch per chunk
};

// the link prologue of the graph phase (assemble.hip, beside links_local)
int links_prologue(ec_session *s, int k, int bbits, bool count_stands, const Scalars &hsc, bool &waited);

// Eligibility and group sizing from (nreads, read_base, k, M, npf, validate); false: the input is
// not one for super-k-mer records.
bool sk2_shape(Sk2Call &c) {
    const int k = c.k;
    if (k < SK_MIN_K || k > 32) return false;
    // k = 31 on reads of M <= 128 windows: 17-window runs stay whole (the entry has the bit)
    c.n17 = k - SK_M + 1 == 17 && c.M <= SK2_FW17_MAXM;
    // read groups: a multiple of the workgroups resident at once when there are more tiles
    // than that (2030 groups of 77 tiles on 768 slots ran 2.64 waves of workgroups, the last
    // one a third idle; 1536 of 102 tiles run 2 full ones), at most RF_MAX_RUNS (k_skrefine)
    const uint64_t ntiles = (c.nreads + 63) / 64, slots = skpart_slots(c.npf, k - SK_M + 1, c.validate, c.n17);
    uint64_t g = std::max<uint64_t>(1, std::min<uint64_t>(ntiles, RF_MAX_RUNS));
    if (g > slots) g = g / slots * slots;
    c.gsize = ((ntiles + g - 1) / g) * 64;
    c.G = (c.nreads + c.gsize - 1) / c.gsize;
    // ((read_base + reads) 2M < 2^32: the events fit 32 bits, and a refined record's position
    // p = (read_base + read) M + window stays below 2^31 -- its bit 31 carries the flip)
    if (c.M > 256 || c.gsize * c.M >= (1ull << 24) || (c.read_base + c.nreads) * 2 * c.M >= (1ull << 32) || kn().no_sk2)
        return false;
    c.mc = sk_cfg(k);
    // records per read ~ 2 M / (w + 1) + 1 on random sequence; 40 % headroom per run
    const double per_read = 2.0 * c.M / (c.mc.w + 1) + 2.0;
    c.cap = (uint64_t)(c.gsize * per_read * 1.4 / SK2_C) + 256;
    c.smask = c.P >= (1ull << 26) ? 255u : 0u;
    // entries a partition wave buffers (EULERHIP_SK2_ELIM: fewer, to test the overflow path)
    c.elim = kn().sk2_elim >= 128 ? (uint32_t)std::min(kn().sk2_elim, SK2_ECAP_W) : (uint32_t)SK2_ECAP_W;
    return true;
}

// overflow / skew / nsolid / ndistinct cleared: what a count that runs again starts from
int clear_count_scalars(Scalars *dsc, hipStream_t st) {
    EC_HIP(hipMemsetAsync(&dsc->overflow, 0, sizeof(unsigned int), st));
    EC_HIP(hipMemsetAsync(&dsc->skew, 0, sizeof(unsigned int), st));
    EC_HIP(hipMemsetAsync(&dsc->nsolid, 0, sizeof(unsigned int), st));
    EC_HIP(hipMemsetAsync(&dsc->ndistinct, 0, sizeof(unsigned long long), st));
    return EC_OK;
}

// a decline: the scalars as phase_count_v2 expects them after its prescan
int sk2_decline(const Sk2Call &c) {
    Scalars *dsc = c.s->scal.as<Scalars>();
    if (c.validate) {  // as begin_call left them: the prescan runs next
        EC_HIP(hipMemsetAsync(dsc, 0, sizeof(Scalars), c.s->stream));
        EC_HIP(hipMemsetAsync(&dsc->bad, 0xFF, sizeof(unsigned long long), c.s->stream));
        return EC_OK;
    }
    return clear_count_scalars(dsc, c.s->stream);
}

// The partition: k_skpart_w over the read groups, the HyperLogLog merge and final, and the
// scalars' read-back queued into hsc (valid after the caller's host wait).
int sk2_partition(Sk2Call &c, Scalars &hsc) {
    ec_session *s = c.s;
    hipStream_t st = s->stream;
    Scalars *dsc = s->scal.as<Scalars>();
    const uint64_t G = c.G;
    const SkPartFn part = skpart_kernel(c.npf, c.mc.w, c.validate, c.n17);
    if (!part) {
        set_error("no k_skpart_w for %d staged KiB, %d windows a block", c.npf, c.mc.w);
        return EC_ERR_STATE;
    }
    EC_CHECK(s->recs.ensure((SK2_C * G * c.cap + SK2_ECAP_W) * 16));  // + the spill records
    EC_CHECK(s->cnt.ensure(SK2_C * G * 4));
    EC_CHECK(s->hll.ensure(G * (1 << HLL_REG_BITS)));
    EC_CHECK(s->ftot.ensure((1 << HLL_REG_BITS) * 4));
    unsigned int *hreg = s->ftot.as<unsigned int>();
    // (validate: the call's first kernel -- the scalars are as begin_call, or sk2_decline after an
    // invalid first try, left them; only k_skpart_w writes nrec)
    if (!c.validate) EC_HIP(hipMemsetAsync(&dsc->nrec, 0, sizeof(unsigned long long), st));
    mark(s, 2 * EC_STAGE_COUNT);
    kmark(s, 1, 0);
    auto launch = [&](unsigned lga, unsigned lgb) {  // read groups [lga, lgb)
        part<<<lgb - lga, PT_THREADS, 0, st>>>(c.d_reads, c.d_off, c.nreads, c.mc, c.M, c.gsize, (uint32_t)G, c.cap,
                                               c.smask, s->recs.as<uint4>(), s->cnt.as<unsigned int>(),
                                               s->hll.as<uint8_t>(), &dsc->nrec, &dsc->overflow, &dsc->lens[2],
                                               &dsc->npos, lga, c.elim);
    };
    // Host input (s->pipe): one launch per arrived chunk, over the groups whose reads it completes
    c.chunked = s->pipe.active && s->pipe.done < s->pipe.nchunks;
    if (!c.chunked) {
        EC_CHECK(pipe_all(s));
        launch(0, (unsigned)G);
    } else {
        unsigned lga = 0;
        for (int pc = 0; pc < s->pipe.nchunks; pc++) {
            const unsigned lgb = pc + 1 == s->pipe.nchunks
                                     ? (unsigned)G
                                     : (unsigned)std::min<uint64_t>(G, s->pipe.ravail[pc] / c.gsize);
            if (lgb <= lga) continue;
            EC_CHECK(pipe_upto(s, pc));
            launch(lga, lgb);
            lga = lgb;
        }
    }
    kmark(s, 1, 1);
    EC_HIP(hipMemsetAsync(hreg, 0, (1 << HLL_REG_BITS) * 4, st));
    k_hll_merge<<<dim3((1 << HLL_REG_BITS) / 256, TOT_SLICES), 256, 0, st>>>(s->hll.as<uint8_t>(), G, hreg);
    k_hll_final<<<1, 1024, 0, st>>>(hreg, HLL_REG_BITS, &dsc->est);
    return d2h(s, &hsc, dsc, sizeof(Scalars), st);
}

// The refine into 2^bb fixed-capacity final buckets of fc records each, and the buckets' bounds.
// A bucket gathers whole minimizers (each ~coverage records): ~13 % spread at the headline
// size (62 minimizers a bucket), so twice the mean: fcap = 2 NR / buckets + 1024 (sk2_plan).
// It only writes recs2 / fcur / bb2, so it may run on speculation and run again.
int sk2_refine(const Sk2Call &c, int bb, uint64_t fc) {
    ec_session *s = c.s;
    hipStream_t st = s->stream;
    Scalars *dsc = s->scal.as<Scalars>();
    const uint64_t nb = 1ull << bb;
    EC_CHECK(s->recs2.ensure(nb * fc * 16));
    EC_CHECK(s->fcur.ensure(nb * 8));
    EC_CHECK(s->bb2.ensure(nb * 16));
    EC_HIP(hipMemsetAsync(s->fcur.p, 0, nb * 8, st));
    unsigned rs = 8;
    if (kn().refine_rs) rs = (unsigned)std::max(1, kn().refine_rs);
    rs = (unsigned)std::min<uint64_t>(rs, c.G);
    kmark(s, 4, 0);
    k_skrefine<<<dim3((unsigned)SK2_C, rs), BUCKET_THREADS, 0, st>>>(
        s->recs.as<uint4>(), s->cnt.as<unsigned int>(), (uint32_t)c.G, c.cap, bb, s->recs2.as<uint4>(), fc,
        s->fcur.as<unsigned long long>(), &dsc->skew, c.M, c.gsize, c.read_base, c.k);
    kmark(s, 4, 1);
    unsigned long long *b0 = s->bb2.as<unsigned long long>();
    k_fixed_bounds<<<grid_for(nb, 256), 256, 0, st>>>(s->fcur.as<unsigned long long>(), nb, fc, b0, b0 + nb);
    return EC_OK;
}

// what the partition's scalars decide about the bucket count
struct Sk2Plan {
    bool ok = false;            // false: the estimate asks for window records (phase_count_v2)
    bool skfilt = false;        // k_skdedup + k_skbucket_filt behind the seen-twice filter
    int bbits = 0;              // 2^bbits final buckets
    unsigned int slots = 0;     // of a bucket's LDS table (1024: k_skbucket3)
    uint64_t fcap = 0;          // records a final bucket holds
    bool refine_stood = false;  // the speculative refine (sp) ran with this plan
};

// The plan from the distinct estimate, the solid limit and the partition's record count.
// sp: the plan the refine was launched with on speculation, null: none was.  Host arithmetic only.
Sk2Plan sk2_plan(double est, long long limit, uint64_t nrec, const ec_session::SkSpec *sp) {
    Sk2Plan p;
    const BucketPlan plan = plan_buckets(est, limit);
    // error-rich input (the estimate asks for the seen-twice filter): super-k-mer buckets behind
    // the filter (k_skbucket_filt) while a bucket's distinct keys stay within its 2^16 filter
    // cells (limit >= 1); otherwise window records with count_part.h's filter
    p.skfilt = plan.part && plan.filt && limit >= 1 && kn().sk_filt != 0 &&
               est / (double)(1ull << SK2_BBITS) <= 16000.0;
    p.ok = plan.part && (!plan.filt || p.skfilt);
    if (!p.ok) return p;
    // up to 2^SK2_BBITS buckets of <= 1100 estimated keys (2048-slot tables: two workgroups per
    // CU).  Measured: 16384 buckets of 1024 slots (three workgroups per CU) were not faster, and
    // small tables need lds_insert to count claims after the CAS (reservations of up to 1024
    // racing lanes overshoot), which cost 8 % in every table
    // (<= 800 estimated keys a bucket: the estimate is +-3 %, and a bucket past ~1100 keys makes
    // both the count and the graph phase's probes measurably slower -- headline A/B 8192 against
    // 4096 buckets: k_skbucket 1.65 / 2.37 ms, links 0.56 / 1.07 ms)
    p.bbits = SK2_CBITS;
    // k_skbucket3 (three workgroups per CU, 1024-slot tables) while its buckets stay at <= 380
    // estimated keys; larger inputs take k_skbucket's 2048- / 4096-slot tables
    const bool b3 = !p.skfilt && !kn().no_skb3 && est / (double)(1ull << SK2_BBITS) <= 380.0;
    const double per_bucket = b3 ? 380.0 : 800.0;
    while (p.bbits < SK2_BBITS && est / (double)(1ull << p.bbits) > per_bucket) p.bbits++;
    if (p.skfilt) p.bbits = SK2_BBITS;
    p.slots = p.skfilt ? 2048u : b3 ? 1024u : est / (double)(1ull << p.bbits) > 1100.0 ? 4096u : 2048u;
    p.fcap = nrec * 2 / (1ull << p.bbits) + 1024;
    p.refine_stood = sp && sp->bbits == p.bbits && sp->fcap >= p.fcap && sp->fcap <= p.fcap + p.fcap / 8;
    if (p.refine_stood)
        p.fcap = sp->fcap;  // the speculative refine stands
    else
        p.fcap += p.fcap / 16;  // (headroom: the next call of this shape keeps the plan)
    return p;
}

// The bucket count for one parity of k: k_skdedup + k_skbucket_filt, k_skbucket3 or
// k_skbucket<2048 | 4096> by the plan.  Records are deduplicated per bucket before their windows
// are rolled out (k_skbucket3 / k_skbucket: 10x fewer k-mer inserts than one per record window on
// the headline).  marked: bmark holds the buckets' first dense ids.
template <bool EVEN>
int sk2_buckets_k(const Sk2Call &c, const Sk2Plan &pl, unsigned long long *dbg, bool &marked) {
    ec_session *s = c.s;
    hipStream_t st = s->stream;
    Scalars *dsc = s->scal.as<Scalars>();
    const uint64_t Bk = 1ull << pl.bbits;
    const int k = c.k;
    const uint32_t M = c.M;
    const double inv_m = 1.0 / M;
    const uint4 *recs2 = s->recs2.as<uint4>();
    const unsigned long long *bbeg = s->bb2.as<unsigned long long>(), *bend = bbeg + Bk;
    // (after a bucket's records and their bounds: what every bucket kernel counts into)
#define EC_SK2_COUNT_ARGS                                                                                        \
    k, M, inv_m, c.limit, s->dkey.as<unsigned long long>(), s->dcnt.as<unsigned int>(),                          \
        s->dfc.as<unsigned long long>(), s->dft.as<unsigned long long>(),                                        \
        s->no_index ? nullptr : s->sub.as<SubSlot>(), &dsc->nsolid, &dsc->ndistinct, &dsc->overflow
    if (pl.skfilt) {
        constexpr int NTF = 512;
        // (the table takes up to 2047 keys; the prediction runs ~10 % high.  ecoli10m_err's
        // fullest bucket: 1525 predicted, 1485 inserted)
        const unsigned int max_keys = kn().skf_keys > 0 ? (unsigned int)kn().skf_keys : 1900u;
        // (round 4 measured a record merge inside the filter kernel on ecoli10m_err: its 1535-entry
        // tables filled -- up to 915 records a bucket rejected -- and its 131 KB of LDS held one
        // workgroup per CU: compact 8.26 ms against 7.75 without it; round 5 merges in a kernel
        // of its own, k_skdedup, EULERHIP_SKF_MERGE=0 the filter alone.
        // No tile planning here: measured on ecoli10m_err the planned tiles left more chains,
        // 11.2 M against 10.9 M -- its graph is cut by error branches, not by tile edges)
        unsigned int *bm = nullptr;
        if (kn().skf_merge != 0) {
            // the bucket's duplicate records merged first (k_skdedup), the filter on the merged ones
            // (bucket b's merged records at its refine region [bbeg[b], ..): Bk x fcap records)
            EC_CHECK(s->skm_rec.ensure(Bk * pl.fcap * sizeof(uint4)));
            EC_CHECK(s->skm_ev.ensure(Bk * pl.fcap * sizeof(uint2)));
            EC_CHECK(s->skm_end.ensure(Bk * 8));
            uint4 *mrec = s->skm_rec.as<uint4>();
            uint2 *mev = s->skm_ev.as<uint2>();
            unsigned long long *mend = s->skm_end.as<unsigned long long>();
            const unsigned int claim_cap = kn().sk2_claim > 0 ? (unsigned int)kn().sk2_claim : ~0u;
            // (4096-entry tables, 1024 threads, one workgroup per CU: compact 2.87-2.92 ms on
            // ecoli10m_err against 3.03-3.06 with 2560 entries and two workgroups per CU)
            if (kn().skf_merge != 2)
                k_skdedup<4096, 1024><<<(unsigned)Bk, 1024, 0, st>>>(recs2, bbeg, bend, k, M, inv_m, mrec, mev, mend,
                                                                     claim_cap, dbg);
            else
                k_skdedup<2560, 512><<<(unsigned)Bk, 512, 0, st>>>(recs2, bbeg, bend, k, M, inv_m, mrec, mev, mend,
                                                                   claim_cap, dbg);
            k_skbucket_filt<2048, NTF, EVEN, true><<<(unsigned)Bk, NTF, 0, st>>>(mrec, bbeg, mend, EC_SK2_COUNT_ARGS,
                                                                                 max_keys, dbg, bm, mev);
        } else {
            k_skbucket_filt<2048, NTF, EVEN><<<(unsigned)Bk, NTF, 0, st>>>(recs2, bbeg, bend, EC_SK2_COUNT_ARGS,
                                                                           max_keys, dbg, bm);
        }
        marked = bm != nullptr;
    } else if (pl.slots == 1024) {
        constexpr int NT3 = 512;
        const unsigned int claim_cap = kn().sk2_claim > 0 ? (unsigned int)kn().sk2_claim : ~0u;
        // bucket starts for the tile ranking: one bit per dense id
        // (a whole number of 256-B lines: the runtime fills an odd tail in a second launch)
        const size_t words = (Bk * pl.slots / 32 + 2 + 63) & ~size_t(63);
        EC_CHECK(s->bmark.ensure(words * 4));
        EC_HIP(hipMemsetAsync(s->bmark.p, 0, words * 4, st));
        unsigned int *bm = s->bmark.as<unsigned int>();
        // (EULERHIP_SK2_STATS: the instantiation with the shader-clock ticks)
        const auto b3 = dbg ? &k_skbucket3<1024, 1664, NT3, EVEN, true> : &k_skbucket3<1024, 1664, NT3, EVEN>;
        b3<<<(unsigned)Bk, NT3, 0, st>>>(recs2, bbeg, bend, EC_SK2_COUNT_ARGS, dbg, claim_cap, bm);
        marked = true;
    } else if (pl.slots == 2048) {
        k_skbucket<2048, 3072, 1, EVEN><<<(unsigned)Bk, BUCKET_THREADS, 0, st>>>(recs2, bbeg, bend, EC_SK2_COUNT_ARGS,
                                                                                 dbg);
    } else {
        k_skbucket<4096, 2048, 1, EVEN><<<(unsigned)Bk, BUCKET_THREADS, 0, st>>>(recs2, bbeg, bend, EC_SK2_COUNT_ARGS,
                                                                                 dbg);
    }
#undef EC_SK2_COUNT_ARGS
    return EC_OK;
}

// super-k-mers -> bucket tables.  dbg: the statistics block of EULERHIP_SK2_STATS (distinct
// records, flushes and windows rolled out), null without it
int sk2_buckets(const Sk2Call &c, const Sk2Plan &pl, unsigned long long *&dbg, bool &marked) {
    marked = false;
    dbg = nullptr;
    if (kn().sk2_stats) {
        EC_CHECK(c.s->tmp.ensure(128));
        dbg = c.s->tmp.as<unsigned long long>();
        EC_HIP(hipMemsetAsync(dbg, 0, 128, c.s->stream));
    }
    return (c.k & 1) ? sk2_buckets_k<false>(c, pl, dbg, marked) : sk2_buckets_k<true>(c, pl, dbg, marked);
}

// EULERHIP_SK2_STATS: the bucket kernels' statistics block read back and printed (stderr)
int sk2_print_stats(const Sk2Call &c, const Sk2Plan &pl, const unsigned long long *dbg, uint64_t NR) {
    ec_session *s = c.s;
    const uint64_t Bk = 1ull << pl.bbits;
    unsigned long long h[16];
    EC_CHECK(d2h(s, h, dbg, 128, s->stream));
    EC_CHECK(host_sync(s, s->stream));
    const double nw = (double)Bk * ((pl.slots == 1024 ? 512 : BUCKET_THREADS) / 64);  // waves
    if (pl.skfilt)
        fprintf(stderr, "k_skbucket_filt: %llu buckets: max distinct est %llu, max predicted inserts %llu, max "
                        "seen-twice cells %llu, max records %llu; refused by the predictor %llu, tables filled "
                        "%llu, most keys inserted %llu; most merged records %llu, most past the claim cap %llu, "
                        "merged records %llu of %llu\n",
                (unsigned long long)Bk, h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8], h[9],
                (unsigned long long)NR);
    if (pl.slots == 1024)
        fprintf(stderr, "k_skbucket3: %llu buckets, most distinct records in a bucket %llu\n",
                (unsigned long long)Bk, h[3]);
    fprintf(stderr, "k_skbucket per wave (shader clocks): records phase canon %.0f probe %.0f (%.1f iterations) "
                    "post %.0f barrier %.0f over %.1f rounds; roll-out %.0f barrier %.0f\n",
            h[8] / nw, h[9] / nw, h[11] / nw, h[10] / nw, h[12] / nw, h[13] / nw, h[14] / nw, h[15] / nw);
    fprintf(stderr, "k_skbucket: %llu records, %llu distinct in %llu flushes (%.2f / bucket), %llu windows rolled "
                    "(positions %llu); block-us: init %.0f records %.0f sort %.0f roll-out %.0f finish %.0f\n",
            (unsigned long long)NR, h[0], h[1], (double)h[1] / Bk, h[2], (unsigned long long)c.P, h[3] / 100.0,
            h[4] / 100.0, h[5] / 100.0, h[6] / 100.0, h[7] / 100.0);
    return EC_OK;
}

// Super-k-mer records for 21 <= k <= 32 (called by phase_count_v2 after its prescan).  done =
// false when the input does not qualify, the distinct estimate asks for the seen-twice filter
// beyond its cells, or a run / bucket / table outgrew its capacity: phase_count_v2 then counts
// with window records.
// validate: no k_prescan ran (phase_count_v2's fast path): M and npf come from the first read,
// the partition checks the input and counts the windows; *invalid = the input does not meet
// the prescan's conditions (the caller then takes the prescan path).
int phase_count_sk2(ec_session *s, const uint8_t *d_reads, const uint64_t *d_off, uint64_t nreads,
                    uint64_t read_base, int k, long long limit, uint32_t M, uint64_t P, int npf, unsigned int &U,
                    SolidIndex &sidx, bool &done, bool validate = false, bool *invalid = nullptr) {
    done = false;
    if (invalid) *invalid = false;
    Sk2Call c{s, d_reads, d_off, nreads, read_base, k, limit, M, P, npf, validate};
    if (!sk2_shape(c)) return EC_OK;
    hipStream_t st = s->stream;
    Scalars *dsc = s->scal.as<Scalars>();
    Scalars hsc;
    const bool verbose = kn().verbose;

    // ---- partition, and the refine on speculation ---------------------------------------------
    EC_CHECK(sk2_partition(c, hsc));
    // the previous call's plan for an input of this shape (a stream of equal batches, the bench's
    // steps) runs the refine while the host waits for the scalars -- the host's wake-up and the
    // plan below overlap the refine instead of idling the device (~40 us a call); a plan that
    // turns out different launches the refine again (it only writes recs2 / fcur / bb2)
    const auto sp = s->skspec;
    const bool spec = sp.valid && sp.G == c.G && sp.cap == c.cap && sp.nreads == nreads && sp.read_base == read_base &&
                      sp.M == M && sp.k == k && !c.chunked && kn().no_spec == 0;
    s->skspec.valid = false;
    if (spec) {
        if (!s->rd_ev) EC_HIP(hipEventCreateWithFlags(&s->rd_ev, hipEventDisableTiming));
        EC_HIP(hipEventRecord(s->rd_ev, st));
        EC_CHECK(sk2_refine(c, sp.bbits, sp.fcap));
        EC_CHECK(host_wait(s, s->rd_ev));
    } else {
        EC_CHECK(host_sync(s, st));
    }
    if (validate) {
        if (hsc.lens[2]) {  // a read of another length, a byte outside ACGT, an oversized tile
            if (verbose) fprintf(stderr, "count_sk2: input needs the prescan\n");
            if (invalid) *invalid = true;
            return sk2_decline(c);
        }
        c.P = hsc.npos;
    }
    if (hsc.overflow) {  // a run outgrew its capacity
        if (verbose) fprintf(stderr, "count_sk2: partition run overflow (cap %llu)\n", (unsigned long long)c.cap);
        return sk2_decline(c);
    }

    // ---- plan; the refine as planned unless the speculative one stands ------------------------
    const double est = hsc.est * (c.smask + 1.0);
    const uint64_t NR = hsc.nrec;
    Sk2Plan pl = sk2_plan(est, limit, NR, spec ? &sp : nullptr);
    if (!pl.ok) return sk2_decline(c);
    if (!pl.refine_stood) {
        if (spec && verbose)
            fprintf(stderr, "count_sk2: refine plan changed (bits %d -> %d), refined again\n", sp.bbits, pl.bbits);
        EC_CHECK(sk2_refine(c, pl.bbits, pl.fcap));
    }
    // (valid, G, cap, nreads, read_base, fcap, M, k, bbits)
    s->skspec = ec_session::SkSpec{true, c.G, c.cap, nreads, read_base, pl.fcap, M, k, pl.bbits};
    mark(s, 2 * EC_STAGE_COUNT + 1);

    // ---- super-k-mers -> bucket tables --------------------------------------------------------
    mark(s, 2 * EC_STAGE_COMPACT);
    const uint64_t Bk = 1ull << pl.bbits, umax = Bk * pl.slots;
    EC_CHECK(s->dkey.ensure(umax * 8));
    EC_CHECK(s->dcnt.ensure(umax * 4));
    EC_CHECK(s->dfc.ensure(umax * 8));
    EC_CHECK(s->dft.ensure(umax * 8));
    EC_CHECK(s->sub.ensure(umax * sizeof(SubSlot)));
    bool b3_marked = false;
    // (a second pass when a final bucket outgrew fcap and the capacity the refine measured is in reach)
    for (int pass = 0; pass < 2; pass++) {
        if (pass) {  // refined again with the measured capacity, then counted again
            EC_CHECK(clear_count_scalars(dsc, st));
            EC_CHECK(sk2_refine(c, pl.bbits, pl.fcap));
        }
        kmark(s, 2, 0);
        unsigned long long *dbg = nullptr;
        EC_CHECK(sk2_buckets(c, pl, dbg, b3_marked));
        if (dbg) EC_CHECK(sk2_print_stats(c, pl, dbg, NR));
        kmark(s, 2, 1);
        mark(s, 2 * EC_STAGE_COMPACT + 1);
        EC_CHECK(d2h(s, &hsc, dsc, sizeof(Scalars), st));
        // the graph phase's first kernels behind the bucket kernel while the host waits for the
        // solid count, only on a first pass whose speculative refine stood (a stream of like batches)
        bool waited = false;
        EC_CHECK(links_prologue(s, k, pl.bbits, !pass && pl.refine_stood && !pl.skfilt && !dbg, hsc, waited));
        if (!waited) EC_CHECK(host_sync(s, st));
        if (!hsc.skew || pass) break;
        // a final bucket past fcap: a repeat family's minimizers (copies x coverage records each) on an
        // input whose buckets hold a few thousand records.  k_skrefine's cursors counted every record,
        // so the fullest bucket's need is known: refined and counted once more with that capacity
        // while it stays within 4x the plan's and 1 GiB of records, instead of leaving the super-k-mer
        // path for the whole call (extreme skew still does, below)
        std::vector<unsigned long long> hcur(Bk);
        EC_CHECK(d2h(s, hcur.data(), s->fcur.p, Bk * 8, st));
        EC_CHECK(host_sync(s, st));
        const uint64_t need = *std::max_element(hcur.begin(), hcur.end());
        if (need <= pl.fcap || need > 4 * pl.fcap || Bk * need * 16 > (1ull << 30)) break;
        if (verbose)
            fprintf(stderr, "count_sk2: final bucket overflow (fcap %llu), refined again with capacity %llu\n",
                    (unsigned long long)pl.fcap, (unsigned long long)need);
        pl.fcap = need;  // (the speculative plan keeps the planned capacity: the next call measures its own)
    }
    if (hsc.overflow || hsc.skew) {  // a final bucket or an LDS table overflowed
        if (verbose)
            fprintf(stderr, "count_sk2: %s overflow (%llu buckets, %u slots, est %.0f, fcap %llu)\n",
                    hsc.skew ? "final bucket" : "table", (unsigned long long)Bk, pl.slots, est,
                    (unsigned long long)pl.fcap);
        s->stats.table_retries++;
        return sk2_decline(c);
    }
    done = true;
    s->bmark_ok = b3_marked;
    s->stats.n_positions = c.P;
    s->stats.n_distinct_est = (uint64_t)llround(est);
    s->stats.record_bytes = 16;
    s->stats.n_records = NR;
    s->stats.count_path = EC_PATH_PARTITIONED;
    s->stats.count_variant = 3;
    s->stats.n_buckets = (uint32_t)Bk;
    s->stats.table_capacity = umax;
    sidx = SolidIndex{};
    sidx.sub = s->sub.as<SubSlot>();
    sidx.bbits = pl.bbits;
    sidx.slots = pl.slots;
    sidx.sk = 1;
    sidx.mc = c.mc;
    sidx.npb = nullptr;
    U = hsc.nsolid;
    s->stats.n_distinct = hsc.ndistinct;
    s->stats.n_solid = U;
    return check_node_ids(U);
}

// count_v2.h: the partitioned count of N-free reads of one length without the histogram
// upsweep.  ok = false (and nothing decided) when the input does not qualify or a run / final
// bucket outgrew its fixed capacity: phase_count then takes count_part.h's exact path.
int phase_count_v2(ec_session *s, const uint8_t *d_reads, const uint64_t *d_off, uint64_t nreads, uint64_t read_base,
                   int k, long long limit, bool allow_sk2, unsigned int &U, SolidIndex &sidx, bool &ok) {
    ok = false;
    hipStream_t st = s->stream;
    Scalars *dsc = s->scal.as<Scalars>();
    Scalars hsc;
    // read groups of whole 64-read wave tiles, at most 2048 (k_refine2 run tables)
    const uint64_t ntiles = (nreads + 63) / 64;
    uint64_t gmax = RF_MAX_RUNS;
    uint64_t G = std::max<uint64_t>(1, std::min<uint64_t>(ntiles, gmax));
    const uint64_t gsize = ((ntiles + G - 1) / G) * 64;
    G = (nreads + gsize - 1) / gsize;
    auto npf_of = [](uint64_t lall) {  // 16-B chunks of a 64-read wave tile -> staged KiB per wave
        const uint64_t need16 = (64ull * lall + 30 + 15) / 16;
        return need16 <= 4 * 64 ? 4 : need16 <= 7 * 64 ? 7 : need16 <= 10 * 64 ? 10 : 0;
    };
    // super-k-mer fast path without the prescan (count_sk2.h, k_skpart_w<., ., true>): the
    // read length of the first read; the partition checks the rest
    if (allow_sk2 && k >= SK_MIN_K && k <= 32 && !kn().no_sk2) {
        uint64_t L = s->lc_L;  // (only a length the fast path then validates is reused)
        if (s->pipe.active) {
            L = s->pipe.first_len;  // host input: the host knows it
        } else if (!(L >= (uint64_t)k && npf_of(L) && s->lc_off == d_off && s->lc_n == nreads)) {
            uint64_t o2[2] = {0, 0};
            EC_CHECK(d2h(s, o2, d_off, 16, st));
            EC_CHECK(host_sync(s, st));
            L = o2[1] - o2[0];
        }
        s->lc_L = 0;  // cached again below only once the partition has validated it
        const int npf = npf_of(L);
        if (L >= (uint64_t)k && npf) {
            const uint32_t M = (uint32_t)(L - k + 1);
            bool done = false, invalid = false;
            mark(s, 2 * EC_STAGE_PRESCAN);  // (no prescan: the stage stays empty)
            mark(s, 2 * EC_STAGE_PRESCAN + 1);
            EC_CHECK(phase_count_sk2(s, d_reads, d_off, nreads, read_base, k, limit, M, nreads * M, npf, U, sidx, done,
                                     true, &invalid));
            if (done) {  // k_skpart_w<., ., true> checked every read against L
                if (!s->pipe.active) s->lc_off = d_off, s->lc_n = nreads, s->lc_L = L;
                ok = true;
                return EC_OK;
            }
            if (!invalid) allow_sk2 = false;  // the estimate or a capacity declined: window records
        }
    }
    EC_CHECK(pipe_all(s));
    mark(s, 2 * EC_STAGE_PRESCAN);
    kmark(s, 0, 0);
    k_prescan<<<(unsigned)G, 256, 0, st>>>(d_reads, d_off, nreads, k, gsize, &dsc->npos, &dsc->bad, dsc->lens);
    kmark(s, 0, 1);
    mark(s, 2 * EC_STAGE_PRESCAN + 1);
    EC_CHECK(d2h(s, &hsc, dsc, sizeof(Scalars), st));
    EC_CHECK(host_sync(s, st));
    EC_CHECK(check_alphabet(d_reads, hsc.bad));
    const unsigned int lmax = hsc.lens[0], lmin = ~hsc.lens[1], lall = hsc.lens[3];
    const uint64_t P = hsc.npos;
    if (hsc.lens[2] || P == 0 || lmax != lmin) return EC_OK;  // N, no windows, several lengths
    const uint32_t M = lmax - (uint32_t)k + 1;
    int ibits = 1;
    while ((1ull << ibits) < M) ibits++;
    if (ibits > 15 || nreads + read_base > (1ull << (31 - ibits)) || 2ull * M - 1 > MAX_LOCAL_EVENT) return EC_OK;
    const int npf = npf_of(lall);
    if (!npf) return EC_OK;
    if (allow_sk2) {  // super-k-mer records (count_sk2.h) unless window records are asked for
        bool done = false;
        EC_CHECK(phase_count_sk2(s, d_reads, d_off, nreads, read_base, k, limit, M, P, npf, U, sidx, done));
        if (done) {
            ok = true;
            return EC_OK;
        }
    }

    // 10-byte partition records (count_v2.h R10) where the hashed-key remnant and the
    // group-relative meta fit 80 bits (large inputs; EULERHIP_V2_R10 = 1 / 0 forces / disables)
    auto nbits = [](uint64_t x) {  // bits of the values 0 .. x - 1
        int b = 0;
        while ((1ull << b) < x) b++;
        return b;
    };
    const int r10env = kn().v2_r10;
    const bool r10 = r10env != 0 && (r10env == 1 || P >= (1ull << 26)) && k >= 16 &&
                     (2 * k - PT_CBITS) + std::max(0, nbits(gsize) + 1 + ibits - 16) <= 64;

    // ---- partition into fixed-capacity (coarse bucket, group) runs -------------------------
    constexpr uint64_t C = 1ull << PT_CBITS;
    const uint64_t cap = (gsize * M * 5 / 4 + C - 1) / C + 128;
    EC_CHECK(s->recs.ensure((C * G * cap + PT_REC) * 12));  // + the spill records
    EC_CHECK(s->cnt.ensure(C * G * 4));
    EC_CHECK(s->hll.ensure(G * (1 << HLL_REG_BITS)));
    EC_CHECK(s->ftot.ensure((1 << HLL_REG_BITS) * 4));
    unsigned long long *rkeys = s->recs.as<unsigned long long>();
    unsigned int *rmeta = reinterpret_cast<unsigned int *>(rkeys + C * G * cap + PT_REC);
    // HyperLogLog over a 1/256 sample of the key space on large inputs (~2 % error from 5·10^5
    // sampled keys up; the estimate only sizes the buckets)
    const uint32_t smask = P >= (1ull << 26) ? 255u : 0u;
    unsigned int *hreg = s->ftot.as<unsigned int>();
    mark(s, 2 * EC_STAGE_COUNT);
    kmark(s, 1, 0);
#define EC_PARTITION(NPF, HI, R10)                                                                            \
    k_partition<NPF, HI, R10><<<(unsigned)G, PT_THREADS, 0, st>>>(d_reads, d_off, nreads, k, M, gsize, (uint32_t)G, \
                                                                   cap, ibits, read_base, smask, rkeys, rmeta,        \
                                                                   s->cnt.as<unsigned int>(),                         \
                                                                   s->hll.as<uint8_t>(), &dsc->overflow)
#define EC_PARTITION_R(NPF, HI)        \
    if (r10)                           \
        EC_PARTITION(NPF, HI, true);   \
    else                               \
        EC_PARTITION(NPF, HI, false)
    if (k >= 17) {
        if (npf == 4) EC_PARTITION_R(4, true);
        else if (npf == 7) EC_PARTITION_R(7, true);
        else EC_PARTITION_R(10, true);
    } else {
        if (npf == 4) EC_PARTITION_R(4, false);
        else if (npf == 7) EC_PARTITION_R(7, false);
        else EC_PARTITION_R(10, false);
    }
#undef EC_PARTITION_R
#undef EC_PARTITION
    kmark(s, 1, 1);
    EC_HIP(hipMemsetAsync(hreg, 0, (1 << HLL_REG_BITS) * 4, st));
    k_hll_merge<<<dim3((1 << HLL_REG_BITS) / 256, TOT_SLICES), 256, 0, st>>>(s->hll.as<uint8_t>(), G, hreg);
    k_hll_final<<<1, 1024, 0, st>>>(hreg, HLL_REG_BITS, &dsc->est);
    EC_CHECK(d2h(s, &hsc, dsc, sizeof(Scalars), st));
    EC_CHECK(host_sync(s, st));
    if (hsc.overflow) return EC_OK;  // a run outgrew its capacity (extreme skew)
    const double est = hsc.est * (smask + 1.0);
    BucketPlan plan = plan_buckets(est, limit);
    if (!plan.part) return EC_OK;
    plan.bbits = std::max(plan.bbits, PT_CBITS);
    const int bbits = plan.bbits;
    const uint64_t Bk = 1ull << bbits;

    // ---- refine into fixed-capacity final buckets -------------------------------------------
    const uint64_t fcap = P * 5 / 4 / Bk + 1024;
    EC_CHECK(s->recs2.ensure(Bk * fcap * 12));
    EC_CHECK(s->fcur.ensure(Bk * 8));
    EC_CHECK(s->bb2.ensure(Bk * 16));
    EC_HIP(hipMemsetAsync(s->fcur.p, 0, Bk * 8, st));
    unsigned rs = 8;
    if (kn().refine_rs) rs = (unsigned)std::max(1, kn().refine_rs);
    rs = (unsigned)std::min<uint64_t>(rs, G);
    kmark(s, 4, 0);
#define EC_REFINE(IN10)                                                                                           \
    k_refine2<IN10><<<dim3((unsigned)C, rs), BUCKET_THREADS, 0, st>>>(                                          \
        rkeys, rmeta, s->cnt.as<unsigned int>(), (uint32_t)G, cap, bbits, s->recs2.as<unsigned int>(), fcap,     \
        s->fcur.as<unsigned long long>(), &dsc->skew, k, ibits, gsize, read_base)
    if (r10)
        EC_REFINE(true);
    else
        EC_REFINE(false);
#undef EC_REFINE
    kmark(s, 4, 1);
    unsigned long long *bbeg = s->bb2.as<unsigned long long>(), *bend = bbeg + Bk;
    k_fixed_bounds<<<grid_for(Bk, 256), 256, 0, st>>>(s->fcur.as<unsigned long long>(), Bk, fcap, bbeg, bend);
    mark(s, 2 * EC_STAGE_COUNT + 1);

    // ---- count buckets in LDS tables ----------------------------------------------------------
    mark(s, 2 * EC_STAGE_COMPACT);
    const uint64_t umax = Bk * plan.slots;
    EC_CHECK(s->dkey.ensure(umax * 8));
    EC_CHECK(s->dcnt.ensure(umax * 4));
    EC_CHECK(s->dfc.ensure(umax * 8));
    EC_CHECK(s->dft.ensure(umax * 8));
    EC_CHECK(s->sub.ensure(umax * sizeof(SubSlot)));
    BucketArgs ba = filter_args(plan.filt, plan.pmax);
    ba.bbeg = bbeg;
    ba.bend = bend;
    kmark(s, 2, 0);
    const unsigned int m2 = 2 * M - 1;
    auto p12 = [&](auto &src) { src.ibits = ibits, src.k = k, src.m2 = m2, src.p = s->recs2.as<unsigned int>(); };
    if (r10 && (k & 1)) {  // the refine's key words hold h = bij_fwd(key)
        Rec12PSource<false, true> src;
        p12(src);
        EC_CHECK(launch_bucket(s, src, (unsigned)Bk, plan.slots, limit, ba));
    } else if (r10) {
        Rec12PSource<true, true> src;
        p12(src);
        EC_CHECK(launch_bucket(s, src, (unsigned)Bk, plan.slots, limit, ba));
    } else if (k & 1) {
        Rec12PSource<false> src;
        p12(src);
        EC_CHECK(launch_bucket(s, src, (unsigned)Bk, plan.slots, limit, ba));
    } else {
        Rec12PSource<true> src;
        p12(src);
        EC_CHECK(launch_bucket(s, src, (unsigned)Bk, plan.slots, limit, ba));
    }
    kmark(s, 2, 1);
    mark(s, 2 * EC_STAGE_COMPACT + 1);
    EC_CHECK(d2h(s, &hsc, dsc, sizeof(Scalars), st));
    EC_CHECK(host_sync(s, st));
    if (hsc.overflow || hsc.skew) {  // a final bucket or an LDS table overflowed: redo on the exact path
        EC_HIP(hipMemsetAsync(dsc, 0, sizeof(Scalars), st));
        EC_HIP(hipMemsetAsync(&dsc->bad, 0xFF, sizeof(unsigned long long), st));
        s->stats.table_retries++;
        return EC_OK;
    }
    ok = true;
    s->stats.n_positions = P;
    s->stats.n_distinct_est = (uint64_t)llround(est);
    s->stats.record_bytes = r10 ? 10 : sizeof(Rec12);  // the partition's records (the refine writes 12 B)
    s->stats.n_records = P;
    s->stats.count_path = EC_PATH_PARTITIONED;
    s->stats.count_variant = r10 ? 2 : 1;
    s->stats.n_buckets = (uint32_t)Bk;
    s->stats.table_capacity = umax;
    sidx = SolidIndex{};
    sidx.sub = s->sub.as<SubSlot>();
    sidx.bbits = bbits;
    sidx.slots = plan.slots;
    sidx.sk = 0;
    sidx.npb = plan.filt ? s->bnp.as<uint8_t>() : nullptr;
    sidx.pmax = plan.pmax;
    sidx.bijk = r10 ? k : 0;  // R10 sub-tables hold bij_fwd(key)
    U = hsc.nsolid;
    s->stats.n_distinct = hsc.ndistinct;
    s->stats.n_solid = U;
    return check_node_ids(U);
}

// build:25-42 on the device: count canonical k-mers of reads [0, nreads) (global read ids
// start at read_base), keep those with count > limit as dense arrays dkey/dcnt/dfc/dft (U of
// them) and a SolidIndex over them.
int phase_count(ec_session *s, const uint8_t *d_reads, const uint64_t *d_off, uint64_t nreads, uint64_t read_base,
                int k, long long limit, unsigned flags, unsigned int &U, SolidIndex &sidx) {
    if (nreads + read_base > (1ull << 32)) {
        set_error("global read ids reach %llu >= 2^32", (unsigned long long)(nreads + read_base));
        return EC_ERR_ARG;
    }
    s->stats.n_reads = nreads;
    hipStream_t st = s->stream;
    const unsigned B = 256;
    Scalars *dsc = s->scal.as<Scalars>();
    Scalars hsc;
    if (!(flags & (EC_FLAG_GENERAL | EC_FLAG_WIDE_RECORDS | EC_FLAG_EXACT_COUNT)) && nreads &&
        k <= 32) {
        bool ok = false;
        EC_CHECK(phase_count_v2(s, d_reads, d_off, nreads, read_base, k, limit, !(flags & EC_FLAG_WINDOW_RECORDS), U,
                                sidx, ok));
        if (ok) return EC_OK;
        EC_HIP(hipMemsetAsync(dsc, 0, sizeof(Scalars), st));
        EC_HIP(hipMemsetAsync(&dsc->bad, 0xFF, sizeof(unsigned long long), st));
    }
    EC_CHECK(pipe_all(s));

    // ---- prescan = partition upsweep ------------------------------------------------------
    mark(s, 2 * EC_STAGE_PRESCAN);
    const uint64_t ntiles = (nreads + TILE_READS - 1) / TILE_READS;
    uint64_t maxg = 2048;
    uint64_t ngroups = std::max<uint64_t>(1, std::min<uint64_t>(ntiles, maxg));
    const uint64_t gsize = std::max<uint64_t>(1, (ntiles + ngroups - 1) / ngroups) * TILE_READS;
    ngroups = std::max<uint64_t>(1, (nreads + gsize - 1) / gsize);
    EC_CHECK(s->hist.ensure(ngroups * FINE * 4));
    EC_CHECK(s->hll.ensure(ngroups * (1 << HLL_REG_BITS)));
    EC_CHECK(s->ftot.ensure((FINE + (1 << HLL_REG_BITS)) * 8));
    if (nreads) {
        kmark(s, 0, 0);
        k_upsweep<<<(unsigned)ngroups, TILE_READS, 0, st>>>(d_reads, d_off, nreads, k, gsize, s->hist.as<unsigned int>(),
                                                           s->hll.as<uint8_t>(), &dsc->npos, &dsc->bad, &dsc->maxlocal,
                                                           &dsc->skew, dsc->lens);
        kmark(s, 0, 1);
        EC_HIP(hipMemsetAsync(s->ftot.p, 0, (FINE + (1 << HLL_REG_BITS)) * 8, st));
        k_fine_totals<<<dim3(FINE / 256, TOT_SLICES), 256, 0, st>>>(
            s->hist.as<unsigned int>(), s->hll.as<uint8_t>(), ngroups, s->ftot.as<unsigned long long>(),
            reinterpret_cast<unsigned int *>(s->ftot.as<unsigned long long>() + FINE));
        k_hll_final<<<1, 1024, 0, st>>>(reinterpret_cast<unsigned int *>(s->ftot.as<unsigned long long>() + FINE),
                                        HLL_REG_BITS, &dsc->est);
    }
    mark(s, 2 * EC_STAGE_PRESCAN + 1);
    EC_CHECK(d2h(s, &hsc, dsc, sizeof(Scalars), st));
    EC_CHECK(host_sync(s, st));
    EC_CHECK(check_alphabet(d_reads, hsc.bad));
    const uint64_t P = nreads ? hsc.npos : 0;
    s->stats.n_positions = P;
    const double est = nreads ? hsc.est : 0.0;
    s->stats.n_distinct_est = (uint64_t)llround(est);

    // ---- count + compact ------------------------------------------------------------------
    // partitioned path when every bucket fits an LDS table and local events fit 16 bits
    // error-rich inputs (distinct keys >> solid keys) use the seen-twice filter buckets when a
    // key seen once cannot be solid by count alone (limit >= 1), up to ~32 K distinct per bucket
    // k_bucket_filt also splits a bucket into up to 2^PMAX part tables (large genomes; with
    // limit < 1 -- shard counts, no filter possible -- every key is kept)
    const BucketPlan plan = plan_buckets(est, limit);
    bool part = !(flags & EC_FLAG_GENERAL) && nreads && P && hsc.maxlocal <= MAX_LOCAL_EVENT && !hsc.skew && plan.part;
    const bool filt = part && plan.filt;
    const int pmax = plan.pmax, bbits = plan.bbits;
    const unsigned int slots = plan.slots;
    sidx = SolidIndex{};
    uint64_t umax = 0;
    if (part) {
        // fewest coarse buckets the refine fan-out allows: longer downsweep runs (measured:
        // 128 vs 256 coarse buckets, k_downsweep 5.56 -> 4.98 ms at 10M x 100 bp)
        int fan = 0;
        while ((1 << (fan + 1)) <= REFINE_FANOUT) fan++;
        int cbits = std::min(bbits, std::max(1, bbits - fan));
        const uint64_t Bk = 1ull << bbits, Ck = 1ull << cbits;
        mark(s, 2 * EC_STAGE_COUNT);
        EC_CHECK(s->cnt.ensure(Ck * ngroups * 8));
        EC_CHECK(s->offs.ensure(Ck * ngroups * 8));
        EC_CHECK(s->tot.ensure((Bk + 1) * 8));
        EC_CHECK(s->bstart.ensure((Bk + 1) * 8));
        // compact 12-B records: every read staged and N-free, one read length, events fit
        const unsigned int lmax = hsc.lens[0], lmin = ~hsc.lens[1];
        bool compact = !(flags & EC_FLAG_WIDE_RECORDS) && hsc.lens[2] == 0 && hsc.lens[1] != 0 && lmax == lmin;
        int ibits = 1;
        if (compact) {
            const uint64_t m = (uint64_t)lmax - (uint64_t)k + 1;
            while ((1ull << ibits) < m) ibits++;
            compact = ibits <= 15 && nreads + read_base <= (1ull << (31 - ibits));
        }
        const uint64_t NR = P;  // records
        const size_t rsz = compact ? sizeof(Rec12) : sizeof(Rec);
        s->stats.record_bytes = (uint32_t)rsz;
        s->stats.n_records = NR;
        EC_CHECK(s->recs.ensure(NR * rsz));
        if (bbits > cbits) EC_CHECK(s->recs2.ensure(NR * sizeof(Rec)));  // refine output
        k_coarse<<<grid_for(Ck * ngroups, B, 8192), B, 0, st>>>(s->hist.as<unsigned int>(), ngroups, cbits,
                                                               s->cnt.as<unsigned long long>());
        EC_CHECK(scan_u64(s, s->cnt.as<unsigned long long>(), s->offs.as<unsigned long long>(), Ck * ngroups));
        k_bucket_totals<<<grid_for(Bk + 1, B), B, 0, st>>>(s->ftot.as<unsigned long long>(), bbits,
                                                          s->tot.as<unsigned long long>());
        EC_CHECK(scan_u64(s, s->tot.as<unsigned long long>(), s->bstart.as<unsigned long long>(), Bk + 1));
        // compact records: keys [0, 8P) and meta [8P, 12P) of the first record buffer
        const Store12 c1{s->recs.as<unsigned long long>(), reinterpret_cast<unsigned int *>(s->recs.as<uint8_t>() + P * 8)};
        kmark(s, 1, 0);
        if (compact)
            k_downsweep<Rec12, MakeRec12, Store12><<<(unsigned)ngroups, TILE_READS, 0, st>>>(
                d_reads, d_off, nreads, k, gsize, ngroups, cbits, s->offs.as<unsigned long long>(), c1,
                MakeRec12{read_base, ibits});
        else
            k_downsweep<Rec, MakeRec, Store16><<<(unsigned)ngroups, TILE_READS, 0, st>>>(
                d_reads, d_off, nreads, k, gsize, ngroups, cbits, s->offs.as<unsigned long long>(),
                Store16{s->recs.as<Rec>()}, MakeRec{read_base});
        kmark(s, 1, 1);
        bool second = false;
        if (bbits > cbits) {
            // split every coarse bucket over RS workgroups (>= 4 per CU in flight)
            unsigned rsmax = 8;
            if (kn().refine_rs) rsmax = (unsigned)std::max(1, kn().refine_rs);
            const unsigned RS = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(rsmax, 1024 * rsmax / 8 / Ck));
            EC_CHECK(s->gcur.ensure(Bk * 8));
            EC_HIP(hipMemcpyAsync(s->gcur.p, s->bstart.p, Bk * 8, hipMemcpyDeviceToDevice, st));
            kmark(s, 4, 0);
            if (compact)  // 12-B in, packed 12-B out
                k_refine<Rec12, Store12, Store12P><<<dim3((unsigned)Ck, RS), BUCKET_THREADS, 0, st>>>(
                    c1, Store12P{s->recs2.as<unsigned int>()}, s->bstart.as<unsigned long long>(),
                    s->gcur.as<unsigned long long>(), cbits, bbits);
            else
                k_refine<Rec, Store16, Store16><<<dim3((unsigned)Ck, RS), BUCKET_THREADS, 0, st>>>(
                    Store16{s->recs.as<Rec>()}, Store16{s->recs2.as<Rec>()}, s->bstart.as<unsigned long long>(),
                    s->gcur.as<unsigned long long>(), cbits, bbits);
            kmark(s, 4, 1);
            second = true;
        }
        mark(s, 2 * EC_STAGE_COUNT + 1);
        mark(s, 2 * EC_STAGE_COMPACT);
        umax = Bk * slots;
        EC_CHECK(s->dkey.ensure(umax * 8));
        EC_CHECK(s->dcnt.ensure(umax * 4));
        EC_CHECK(s->dfc.ensure(umax * 8));
        EC_CHECK(s->dft.ensure(umax * 8));
        EC_CHECK(s->sub.ensure(umax * sizeof(SubSlot)));
        kmark(s, 2, 0);
        const BucketArgs ba = filter_args(filt, pmax);
        if (compact && second) {
            const unsigned int m2 = (unsigned int)(2 * ((uint64_t)lmax - k + 1) - 1);
            if (k & 1) {
                Rec12PSource<false> src;
                src.ibits = ibits, src.k = k, src.m2 = m2, src.p = s->recs2.as<unsigned int>();
                EC_CHECK(launch_bucket(s, src, (unsigned)Bk, slots, limit, ba));
            } else {
                Rec12PSource<true> src;
                src.ibits = ibits, src.k = k, src.m2 = m2, src.p = s->recs2.as<unsigned int>();
                EC_CHECK(launch_bucket(s, src, (unsigned)Bk, slots, limit, ba));
            }
        } else if (compact) {
            const unsigned int m2 = (unsigned int)(2 * ((uint64_t)lmax - k + 1) - 1);
            if (k & 1) {
                Rec12Source<false> src;
                src.ibits = ibits, src.k = k, src.m2 = m2, src.key = c1.key, src.meta = c1.meta;
                EC_CHECK(launch_bucket(s, src, (unsigned)Bk, slots, limit, ba));
            } else {
                Rec12Source<true> src;
                src.ibits = ibits, src.k = k, src.m2 = m2, src.key = c1.key, src.meta = c1.meta;
                EC_CHECK(launch_bucket(s, src, (unsigned)Bk, slots, limit, ba));
            }
        } else {
            EC_CHECK(launch_bucket(s, RecSource{second ? s->recs2.as<Rec>() : s->recs.as<Rec>()}, (unsigned)Bk, slots,
                                   limit, ba));
        }
        kmark(s, 2, 1);
        mark(s, 2 * EC_STAGE_COMPACT + 1);
        EC_CHECK(d2h(s, &hsc, dsc, sizeof(Scalars), st));
        EC_CHECK(host_sync(s, st));
        if (hsc.overflow) {  // a bucket outgrew its LDS table: redo on the general path
            part = false;
            s->stats.table_retries++;
            EC_HIP(hipMemsetAsync(&dsc->nsolid, 0, 4, st));
            EC_HIP(hipMemsetAsync(&dsc->ndistinct, 0, 8, st));
            EC_HIP(hipMemsetAsync(&dsc->overflow, 0, 4, st));
        } else {
            sidx.sub = s->sub.as<SubSlot>();
            sidx.bbits = bbits;
            sidx.slots = slots;
            sidx.sk = 0;
            sidx.npb = filt ? s->bnp.as<uint8_t>() : nullptr;
            sidx.pmax = pmax;
            s->stats.count_path = EC_PATH_PARTITIONED;
            s->stats.n_buckets = (uint32_t)Bk;
            s->stats.table_capacity = umax;
        }
    }
    if (!part) {
        uint64_t want = (uint64_t)(std::max<double>(est, 1.0) * 2.2) + 1024;
        want = std::min<uint64_t>(want, 2 * P + 1024);
        uint64_t cap = 1024;
        while (cap < want) cap <<= 1;
        for (int attempt = 0;; attempt++) {
            EC_CHECK(s->table.ensure(cap * sizeof(Slot)));
            mark(s, 2 * EC_STAGE_COUNT);
            k_table_clear<<<grid_for(cap, B, 8192), B, 0, st>>>(s->table.as<Slot>(), cap);
            EC_HIP(hipMemsetAsync(&dsc->overflow, 0, 4, st));
            kmark(s, 3, 0);
            if (nreads)
                k_count<<<grid_for(nreads, B), B, 0, st>>>(d_reads, d_off, nreads, k, s->table.as<Slot>(), cap - 1,
                                                          &dsc->overflow, read_base);
            kmark(s, 3, 1);
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
        s->stats.table_capacity = cap;
        mark(s, 2 * EC_STAGE_COMPACT);
        umax = cap;
        EC_CHECK(s->dkey.ensure(umax * 8));
        EC_CHECK(s->dcnt.ensure(umax * 4));
        EC_CHECK(s->dfc.ensure(umax * 8));
        EC_CHECK(s->dft.ensure(umax * 8));
        EC_CHECK(compact_table(s, s->table.as<Slot>(), cap, (long long)limit, s->dkey.as<unsigned long long>()));
        mark(s, 2 * EC_STAGE_COMPACT + 1);
        EC_CHECK(d2h(s, &hsc, dsc, sizeof(Scalars), st));
        EC_CHECK(host_sync(s, st));
        sidx.table = s->table.as<Slot>();
        sidx.capmask = cap - 1;
        s->stats.count_path = EC_PATH_GENERAL;
    }
    U = hsc.nsolid;
    s->stats.n_distinct = hsc.ndistinct;
    s->stats.n_solid = U;
    return check_node_ids(U);
}

// Owner-side aggregation of exchanged k-mer records (count sum, first-event min) followed by
// the solid filter: the merge step of the sharded path, and the way a gathered solid set is
// loaded for phase_graph (limit = keep all).
// The same on the LDS bucket tables of the fused path (k_bucket over the records sorted by
// bucket): no HBM atomics.  Returns EC_OK with ok = false when a bucket overflows its table.
// minimizer buckets for the merge / load of 21 <= k <= 32 (shard.h OwnerFn)
bool merge_sk(int k) { return k >= SK_MIN_K && k <= 32; }
// 128-bit keys on minimizer owners (the count's minimizer buckets, count_wide.h)
bool merge_wmb(int k) { return k > 32 && k <= WMB_MAX_K && kn().wide_mb != 0; }
OwnerFn owner_fn(int k) {
    OwnerFn f{};
    f.sk = merge_sk(k) ? 1 : 0;
    if (f.sk) f.mc = sk_cfg(k);
    f.wk = merge_wmb(k) ? k : 0;
    return f;
}

// counting sort of n > 0 bin ids (shard.h k_cs_*): perm in midx2, bin starts bstart[0..nbins)
// (end: and bstart[nbins] = n)
int cs_sort(ec_session *s, const unsigned int *bid, uint64_t n, unsigned int nbins, unsigned long long *bstart,
            bool end = false) {
    hipStream_t st = s->stream;
    const unsigned int nch = (unsigned int)((n + CS_CHUNK - 1) / CS_CHUNK);
    EC_CHECK(s->midx2.ensure(std::max<uint64_t>(n, 1) * 4));
    EC_CHECK(s->mbid2.ensure(std::max<uint64_t>(n, 3ull * nbins) * 4));  // (mbid2 is free here)
    unsigned int *tot = s->mbid2.as<unsigned int>(), *incl = tot + nbins, *cur = incl + nbins;
    EC_HIP(hipMemsetAsync(tot, 0, (size_t)nbins * 4, st));
    k_cs_hist<<<nch, 1024, nbins * 4, st>>>(bid, n, nbins, tot);
    EC_CHECK(scan_incl_u32(s, tot, incl, nbins));
    k_cs_starts<<<grid_for(nbins, 256), 256, 0, st>>>(tot, incl, nbins, bstart, cur, end);
    k_cs_scatter<<<nch, 1024, nbins * 4, st>>>(bid, n, nbins, cur, s->midx2.as<unsigned int>());
    return EC_OK;
}

int phase_merge_part(ec_session *s, const Agg *d_agg, uint64_t n, long long limit, unsigned int &U, SolidIndex &sidx,
                     bool &ok, const unsigned int *ids = nullptr, bool allow_sk = true, const XIn *xin = nullptr) {
    // (xin: the received records read in place, ec_merge_owned_from; d_agg unused)
    hipStream_t st = s->stream;
    const unsigned B = 256;
    Scalars *dsc = s->scal.as<Scalars>();
    Scalars hsc;
    ok = false;
    int bbits = 0;
    while (bbits < FINE_BITS && (double)n / (double)(1ull << bbits) > 1100.0) bbits++;
    if ((double)n / (double)(1ull << bbits) > 2200.0) return EC_OK;  // too large for the LDS tables
    const unsigned int nb = 1u << bbits;
    const unsigned int slots = (double)n / (double)nb > 1100.0 ? 4096u : 2048u;
    OwnerFn own = owner_fn(s->k);  // minimizer buckets (own.sk) or key-hash buckets
    if (!allow_sk) own.sk = 0;
    mark(s, 2 * EC_STAGE_COUNT);
    EC_CHECK(s->mbid.ensure(std::max<uint64_t>(n, 1) * 4));
    EC_CHECK(s->mbid2.ensure(std::max<uint64_t>(n, 1) * 4));
    EC_CHECK(s->midx2.ensure(std::max<uint64_t>(n, 1) * 4));
    EC_CHECK(s->bstart.ensure((nb + 1ull) * 8));
    if (!n) EC_HIP(hipMemsetAsync(s->bstart.p, 0, (nb + 1ull) * 8, st));  // (else k_cs_starts writes them all)
    if (n) {
        if (xin)
            k_agg_bucket_ids<XIn><<<grid_for(n, B), B, 0, st>>>(*xin, n, bbits, s->mbid.as<unsigned int>(), own.mc,
                                                               own.sk);
        else
            k_agg_bucket_ids<PlainIn><<<grid_for(n, B), B, 0, st>>>(PlainIn{d_agg}, n, bbits, s->mbid.as<unsigned int>(),
                                                                   own.mc, own.sk);
        // indices by bucket: counting sort (shard.h k_cs_*), buckets 0..nb (nb: filler records)
        EC_CHECK(cs_sort(s, s->mbid.as<unsigned int>(), n, nb + 1, s->bstart.as<unsigned long long>()));
    }
    mark(s, 2 * EC_STAGE_COUNT + 1);
    mark(s, 2 * EC_STAGE_COMPACT);
    const uint64_t umax = (uint64_t)nb * slots;
    EC_CHECK(s->dkey.ensure(umax * 8));
    EC_CHECK(s->dcnt.ensure(umax * 4));
    EC_CHECK(s->dfc.ensure(umax * 8));
    EC_CHECK(s->dft.ensure(umax * 8));
    EC_CHECK(s->sub.ensure(umax * sizeof(SubSlot)));
    // ndistinct, est, overflow, nsolid: one fill (they are adjacent; est is the count's alone)
    static_assert(offsetof(Scalars, nsolid) + 4 - offsetof(Scalars, ndistinct) == 24, "Scalars layout");
    EC_HIP(hipMemsetAsync(&dsc->ndistinct, 0, 24, st));
    kmark(s, 2, 0);
    const int sks = own.sk ? (slots == 2048 ? 11 : 12) : 0;
    bool merge_marked = false;
    if (!ids) s->seg_marks = 0;
    if (ids) {  // gathered solid set: dense ids given (partitioned graph phase)
        const AggDetSource src{d_agg, s->midx2.as<unsigned int>(), ids, sks};
        EC_CHECK(launch_bucket(s, src, nb, slots, limit));
    } else {
        // (minimizer buckets: their first ids marked for the partitioned finish's tiles)
        BucketArgs ba;
        if (own.sk) {
            const size_t words = umax / 32 + 2;
            EC_CHECK(s->bmark.ensure(words * 4));
            EC_HIP(hipMemsetAsync(s->bmark.p, 0, words * 4, st));
            ba.bmark = s->bmark.as<unsigned int>();
        }
        if (xin) {
            const XAggSource src{*xin, s->midx2.as<unsigned int>(), sks};
            EC_CHECK(launch_bucket(s, src, nb, slots, limit, ba));
        } else {
            const AggSource src{d_agg, s->midx2.as<unsigned int>(), sks};
            EC_CHECK(launch_bucket(s, src, nb, slots, limit, ba));
        }
        merge_marked = ba.bmark != nullptr;
    }
    kmark(s, 2, 1);
    mark(s, 2 * EC_STAGE_COMPACT + 1);
    EC_CHECK(d2h(s, &hsc, dsc, sizeof(Scalars), st));
    EC_CHECK(host_sync(s, st));
    if (hsc.overflow) {
        s->stats.table_retries++;
        EC_HIP(hipMemsetAsync(&dsc->overflow, 0, 4, st));
        return EC_OK;
    }
    U = ids ? hsc.ngath : hsc.nsolid;  // ids: the dense ids k_det_ids gave (their count in ngath)
    s->stats.n_distinct = U;
    if (!ids) s->stats.n_distinct = hsc.ndistinct;
    s->stats.n_solid = U;
    s->stats.count_path = EC_PATH_PARTITIONED;
    s->stats.n_buckets = nb;
    s->stats.table_capacity = umax;
    sidx = SolidIndex{};
    sidx.sub = s->sub.as<SubSlot>();
    sidx.bbits = bbits;
    sidx.slots = slots;
    sidx.sk = own.sk;
    if (own.sk) sidx.mc = own.mc;
    EC_CHECK(check_node_ids(U));
    if (merge_marked) s->seg_marks = U;  // (bmark holds this merge's bucket starts, U ids)
    ok = true;
    return EC_OK;
}

int phase_merge(ec_session *s, const Agg *d_agg, uint64_t n, long long limit, unsigned int &U, SolidIndex &sidx,
                const XIn *xin = nullptr, const std::function<int(const Agg *&)> &decode = nullptr) {
    if (!(s->flags & EC_FLAG_GENERAL)) {
        bool ok = false;
        EC_CHECK(phase_merge_part(s, d_agg, n, limit, U, sidx, ok, nullptr, true, xin));
        if (!ok && merge_sk(s->k)) EC_CHECK(phase_merge_part(s, d_agg, n, limit, U, sidx, ok, nullptr, false, xin));
        if (ok) return EC_OK;
    }
    if (xin) EC_CHECK(decode(d_agg));  // the HBM table reads decoded records
    hipStream_t st = s->stream;
    const unsigned B = 256;
    Scalars *dsc = s->scal.as<Scalars>();
    Scalars hsc;
    uint64_t cap = 1024;
    while (cap < (uint64_t)(2.2 * (double)n) + 1024) cap <<= 1;
    for (int attempt = 0;; attempt++) {
        EC_CHECK(s->table.ensure(cap * sizeof(Slot)));
        mark(s, 2 * EC_STAGE_COUNT);
        k_table_clear<<<grid_for(cap, B, 8192), B, 0, st>>>(s->table.as<Slot>(), cap);
        EC_HIP(hipMemsetAsync(&dsc->overflow, 0, 4, st));
        if (n) k_merge_agg<<<grid_for(n, B), B, 0, st>>>(d_agg, n, s->table.as<Slot>(), cap - 1, &dsc->overflow);
        mark(s, 2 * EC_STAGE_COUNT + 1);
        EC_CHECK(d2h(s, &hsc.overflow, &dsc->overflow, 4, st));
        EC_CHECK(host_sync(s, st));
        if (!hsc.overflow) break;
        if (attempt >= 4) {
            set_error("merge table overflow at capacity %llu", (unsigned long long)cap);
            return EC_ERR_CAPACITY;
        }
        cap <<= 2;
        s->stats.table_retries++;
    }
    s->stats.table_capacity = cap;
    mark(s, 2 * EC_STAGE_COMPACT);
    EC_CHECK(s->dkey.ensure(cap * 8));
    EC_CHECK(s->dcnt.ensure(cap * 4));
    EC_CHECK(s->dfc.ensure(cap * 8));
    EC_CHECK(s->dft.ensure(cap * 8));
    EC_HIP(hipMemsetAsync(&dsc->nsolid, 0, 4, st));
    EC_HIP(hipMemsetAsync(&dsc->ndistinct, 0, 8, st));
    EC_CHECK(compact_table(s, s->table.as<Slot>(), cap, limit, s->dkey.as<unsigned long long>()));
    mark(s, 2 * EC_STAGE_COMPACT + 1);
    EC_CHECK(d2h(s, &hsc, dsc, sizeof(Scalars), st));
    EC_CHECK(host_sync(s, st));
    U = hsc.nsolid;
    s->stats.n_distinct = hsc.ndistinct;
    s->stats.n_solid = U;
    s->stats.count_path = EC_PATH_GENERAL;
    sidx = SolidIndex{};
    sidx.table = s->table.as<Slot>();
    sidx.capmask = cap - 1;
    return check_node_ids(U);
}


// partitioned graph phase: the all-gathered solid set with dense ids = position among the
// non-filler records (owner-major), identical on every rank, plus the bucketed lookup index
int phase_load_det(ec_session *s, const Agg *d_agg, uint64_t n, unsigned int &U, SolidIndex &sidx) {
    hipStream_t st = s->stream;
    Scalars *dsc = s->scal.as<Scalars>();
    const unsigned int nblk = (unsigned int)std::max<uint64_t>((n + DET_CHUNK - 1) / DET_CHUNK, 1);
    EC_CHECK(s->rbc.ensure((size_t)nblk * 8));
    EC_CHECK(s->nextR.ensure(std::max<uint64_t>(n, 1) * 4));  // ids (nextR is free until the rank stage)
    unsigned int *bc = s->rbc.as<unsigned int>(), *bs = bc + nblk, *ids = s->nextR.as<unsigned int>();
    // the id count stays on the device (dsc->ngath, read back with phase_merge_part's scalars):
    // the dense arrays are sized for all n records, so no host round trip here
    EC_HIP(hipMemsetAsync(&dsc->ngath, 0, 4, st));
    if (n) {
        k_det_count<Agg><<<nblk, 256, 0, st>>>(d_agg, n, bc);
        EC_CHECK(scan_incl_u32(s, bc, bs, nblk));
        k_det_ids<Agg><<<nblk, 256, 0, st>>>(d_agg, n, bs, ids);
        EC_HIP(hipMemcpyAsync(&dsc->ngath, bs + nblk - 1, 4, hipMemcpyDeviceToDevice, st));
    }
    EC_CHECK(s->dkey.ensure(std::max<uint64_t>(n, 1) * 8));
    EC_CHECK(s->dcnt.ensure(std::max<uint64_t>(n, 1) * 4));
    EC_CHECK(s->dfc.ensure(std::max<uint64_t>(n, 1) * 8));
    EC_CHECK(s->dft.ensure(std::max<uint64_t>(n, 1) * 8));
    bool ok = false;
    EC_CHECK(phase_merge_part(s, d_agg, n, LLONG_MIN, U, sidx, ok, ids));
    // a minimizer bucket past its table (low-complexity sequence: many keys, one minimizer):
    // key-hash buckets instead
    if (!ok && merge_sk(s->k)) EC_CHECK(phase_merge_part(s, d_agg, n, LLONG_MIN, U, sidx, ok, ids, false));
    if (!ok) {
        set_error("gathered solid set of %llu records does not fit the bucketed index", (unsigned long long)n);
        return EC_ERR_CAPACITY;
    }
    (void)dsc;
    return EC_OK;
}

// the same for k > 32: dense arrays in gathered order, HBM lookup table (SolidIndexW)
int phase_load_det_w(ec_session *s, const AggW *d_agg, uint64_t n, unsigned int &U, SolidIndexW &sidx) {
    hipStream_t st = s->stream;
    const unsigned B = 256;
    Scalars *dsc = s->scal.as<Scalars>();
    const unsigned int nblk = (unsigned int)std::max<uint64_t>((n + DET_CHUNK - 1) / DET_CHUNK, 1);
    EC_CHECK(s->rbc.ensure((size_t)nblk * 8));
    EC_CHECK(s->nextR.ensure(std::max<uint64_t>(n, 1) * 4));
    unsigned int *bc = s->rbc.as<unsigned int>(), *bs = bc + nblk, *ids = s->nextR.as<unsigned int>();
    unsigned int tot = 0;
    if (n) {
        k_det_count<AggW><<<nblk, 256, 0, st>>>(d_agg, n, bc);
        EC_CHECK(scan_incl_u32(s, bc, bs, nblk));
        k_det_ids<AggW><<<nblk, 256, 0, st>>>(d_agg, n, bs, ids);
        EC_CHECK(d2h(s, &tot, bs + nblk - 1, 4, st));
        EC_CHECK(host_sync(s, st));
    }
    EC_CHECK(s->dkey.ensure(std::max<uint64_t>(tot, 1) * sizeof(K128)));
    EC_CHECK(s->dcnt.ensure(std::max<uint64_t>(tot, 1) * 4));
    EC_CHECK(s->dfc.ensure(std::max<uint64_t>(tot, 1) * 8));
    EC_CHECK(s->dft.ensure(std::max<uint64_t>(tot, 1) * 8));
    uint64_t cap = 1024;
    while (cap < (uint64_t)(2.2 * (double)tot) + 1024) cap <<= 1;
    for (int attempt = 0;; attempt++) {
        EC_CHECK(s->table.ensure(cap * sizeof(SlotW)));
        mark(s, 2 * EC_STAGE_COUNT);
        k_table_clear_w<<<grid_for(cap, B, 8192), B, 0, st>>>(s->table.as<SlotW>(), cap);
        EC_HIP(hipMemsetAsync(&dsc->overflow, 0, 4, st));
        if (n)
            k_load_det_w<<<grid_for(n, B), B, 0, st>>>(d_agg, n, ids, s->table.as<SlotW>(), cap - 1, s->dkey.as<K128>(),
                                                      s->dcnt.as<unsigned int>(), s->dfc.as<unsigned long long>(),
                                                      s->dft.as<unsigned long long>(), &dsc->overflow);
        mark(s, 2 * EC_STAGE_COUNT + 1);
        unsigned int of = 0;
        EC_CHECK(d2h(s, &of, &dsc->overflow, 4, st));
        EC_CHECK(host_sync(s, st));
        if (!of) break;
        if (attempt >= 4) {
            set_error("load table overflow at capacity %llu", (unsigned long long)cap);
            return EC_ERR_CAPACITY;
        }
        cap <<= 2;
        s->stats.table_retries++;
    }
    U = tot;
    s->stats.n_distinct = tot;
    s->stats.n_solid = tot;
    s->stats.table_capacity = cap;
    sidx.table = s->table.as<SlotW>();
    sidx.capmask = cap - 1;
    sidx.sub = nullptr;
    return EC_OK;
}

// ---- 32 < k <= 63: 128-bit keys (wide.h), general-table counting ---------------------------
int finish_wide(ec_session *s, uint64_t cap, long long limit, unsigned int &U, SolidIndexW &sidx,
                uint64_t ubound = 0) {
    hipStream_t st = s->stream;
    Scalars *dsc = s->scal.as<Scalars>();
    Scalars hsc;
    mark(s, 2 * EC_STAGE_COMPACT);
    // (ubound: at most that many keys -- a merge's records; the table's capacity otherwise)
    const uint64_t ucap = ubound ? std::min<uint64_t>(cap, ubound) : cap;
    EC_CHECK(s->dkey.ensure(std::max<uint64_t>(ucap, 1) * sizeof(K128)));
    EC_CHECK(s->dcnt.ensure(std::max<uint64_t>(ucap, 1) * 4));
    EC_CHECK(s->dfc.ensure(std::max<uint64_t>(ucap, 1) * 8));
    EC_CHECK(s->dft.ensure(std::max<uint64_t>(ucap, 1) * 8));
    EC_HIP(hipMemsetAsync(&dsc->nsolid, 0, 4, st));
    EC_HIP(hipMemsetAsync(&dsc->ndistinct, 0, 8, st));
    EC_CHECK(compact_table(s, s->table.as<SlotW>(), cap, limit, s->dkey.as<K128>()));
    mark(s, 2 * EC_STAGE_COMPACT + 1);
    EC_CHECK(d2h(s, &hsc, dsc, sizeof(Scalars), st));
    EC_CHECK(host_sync(s, st));
    U = hsc.nsolid;
    s->stats.n_distinct = hsc.ndistinct;
    s->stats.n_solid = U;
    s->stats.count_path = EC_PATH_GENERAL;
    s->stats.table_capacity = cap;
    sidx.table = s->table.as<SlotW>();
    sidx.capmask = cap - 1;
    sidx.sub = nullptr;
    return check_node_ids(U);
}

// Partitioned wide count (count_wide.h): upsweep, downsweep, refine and one LDS table per
// bucket, as phase_count for k <= 32.  ok = false (scalars reset) when the input needs the
// HBM table: reads with 'N' or other bytes, tiles over the 40 KB stage, a bucket past its table.
int phase_count_wpart(ec_session *s, const uint8_t *d_reads, const uint64_t *d_off, uint64_t nreads,
                      uint64_t read_base, int k, long long limit, unsigned int &U, SolidIndexW &sidx, bool &ok,
                      bool mb = false, bool *mb_declined = nullptr) {
    ok = false;
    if ((s->flags & EC_FLAG_GENERAL) || !nreads) return EC_OK;
    hipStream_t st = s->stream;
    const unsigned B = 256;
    Scalars *dsc = s->scal.as<Scalars>();
    Scalars hsc;
    auto reset = [&]() -> int {
        EC_HIP(hipMemsetAsync(dsc, 0, sizeof(Scalars), st));
        EC_HIP(hipMemsetAsync(&dsc->bad, 0xFF, sizeof(unsigned long long), st));
        return EC_OK;
    };
    mark(s, 2 * EC_STAGE_PRESCAN);
    const uint64_t ntiles = (nreads + TILE_READS - 1) / TILE_READS;
    uint64_t maxg = 2048;
    uint64_t ngroups = std::max<uint64_t>(1, std::min<uint64_t>(ntiles, maxg));
    const uint64_t gsize = std::max<uint64_t>(1, (ntiles + ngroups - 1) / ngroups) * TILE_READS;
    ngroups = std::max<uint64_t>(1, (nreads + gsize - 1) / gsize);
    constexpr int HR = 1 << HLL_REG_BITS;
    EC_CHECK(s->hist.ensure(ngroups * FINE_W * 4));
    EC_CHECK(s->hll.ensure(ngroups * HR));
    EC_CHECK(s->ftot.ensure((FINE_W + HR) * 8));
    kmark(s, 0, 0);
    // minimizer buckets (count_wide.h k_wbv): every window's minimizer, indexed by its base offset
    uint32_t *wbv = nullptr;
    uint32_t mbM = 0;
    uint32_t *rpack = nullptr, rpack_d = 0;
    if (mb) {  // reads of one length L <= WMB_MAXL only (k_wbv checks the others)
        uint64_t o2[2] = {0, 0};
        EC_CHECK(d2h(s, o2, d_off, 16, st));
        EC_CHECK(host_sync(s, st));
        const uint64_t L = o2[1] - o2[0];
        if (L < (uint64_t)k || L > WMB_MAXL) {
            if (mb_declined) *mb_declined = true;
            return reset();
        }
        mbM = (uint32_t)(L - k + 1);
        EC_HIP(hipMemsetAsync(&dsc->wbv_long, 0, 4, st));
        EC_CHECK(s->wbv.ensure(((nreads + 255) / 256) * 256 * (uint64_t)mbM * 4));
        wbv = s->wbv.as<uint32_t>();
        const unsigned g = (unsigned)((nreads + 63) / 64);
        // large inputs (the third level's run codes): k_wbv also writes the reads as 2-bit codes,
        // from which k_run_codes copies each run's codes
        if (kn().wide_runs != 0 && (uint64_t)nreads * mbM >= (1ull << 26)) {
            rpack_d = (uint32_t)((L + 15) / 16);
            EC_CHECK(s->rpack.ensure((uint64_t)nreads * rpack_d * 4));
            rpack = s->rpack.as<uint32_t>();
        }
        switch (k - SK_M + 1) {  // (WMB_MAX_K = 52: w <= 38)
#define EC_WBV(W) \
    case W: k_wbv<W><<<g, 64, 0, st>>>(d_reads, d_off, nreads, (uint32_t)L, wbv, &dsc->wbv_long, rpack, rpack_d); break;
            EC_WBV(19) EC_WBV(20) EC_WBV(21) EC_WBV(22) EC_WBV(23) EC_WBV(24) EC_WBV(25) EC_WBV(26) EC_WBV(27)
            EC_WBV(28) EC_WBV(29) EC_WBV(30) EC_WBV(31) EC_WBV(32) EC_WBV(33) EC_WBV(34) EC_WBV(35) EC_WBV(36)
            EC_WBV(37) EC_WBV(38)
#undef EC_WBV
            default: set_error("minimizer buckets: k = %d out of range", k); return EC_ERR_ARG;
        }
    }
    // minimizer runs as the partition records (count_wide.h RunWM; EULERHIP_WIDE_RUNS=0: windows)
    const bool runs = mb && kn().wide_runs != 0;
    // HyperLogLog sampled by minimizer past ~6.7e7 positions (as the super-k-mer count)
    const uint32_t hsmask = mb && (uint64_t)nreads * mbM >= (1ull << 26) ? 255u : 0u;
    if (runs)
        k_upsweep_runs<<<(unsigned)ngroups, TILE_READS, 0, st>>>(d_reads, d_off, nreads, k, gsize,
                                                                s->hist.as<unsigned int>(), s->hll.as<uint8_t>(),
                                                                &dsc->npos, &dsc->maxlocal, &dsc->skew, wbv, mbM,
                                                                hsmask);
    else if (mb)
        k_upsweep_w<true><<<(unsigned)ngroups, TILE_READS, 0, st>>>(d_reads, d_off, nreads, k, gsize,
                                                                   s->hist.as<unsigned int>(), s->hll.as<uint8_t>(),
                                                                   &dsc->npos, &dsc->maxlocal, &dsc->skew, dsc->lens,
                                                                   wbv, mbM, hsmask);
    else
        k_upsweep_w<false><<<(unsigned)ngroups, TILE_READS, 0, st>>>(d_reads, d_off, nreads, k, gsize,
                                                                    s->hist.as<unsigned int>(), s->hll.as<uint8_t>(),
                                                                    &dsc->npos, &dsc->maxlocal, &dsc->skew, dsc->lens,
                                                                    nullptr, 0u);
    kmark(s, 0, 1);
    unsigned long long *ftot = s->ftot.as<unsigned long long>();
    EC_HIP(hipMemsetAsync(ftot, 0, (FINE_W + HR) * 8, st));
    EC_HIP(hipMemsetAsync(&dsc->nrec, 0, sizeof(unsigned long long), st));
    k_fine_totals<FINE_W_BITS><<<dim3(FINE_W / 256, TOT_SLICES), 256, 0, st>>>(
        s->hist.as<unsigned int>(), s->hll.as<uint8_t>(), ngroups, ftot, reinterpret_cast<unsigned int *>(ftot + FINE_W),
        &dsc->nrec);
    k_hll_final<<<1, 1024, 0, st>>>(reinterpret_cast<unsigned int *>(ftot + FINE_W), HLL_REG_BITS, &dsc->est);
    mark(s, 2 * EC_STAGE_PRESCAN + 1);
    EC_CHECK(d2h(s, &hsc, dsc, sizeof(Scalars), st));
    EC_CHECK(host_sync(s, st));
    const uint64_t P = hsc.npos;
    const double est = hsc.est * (hsmask + 1.0);
    // Up to 2^FINE_W_BITS buckets of <= 1100 estimated keys in 3328-slot tables (156 KB: one
    // workgroup per CU), sized exactly by the fine histogram.  Past that (~1.8e7 keys: config
    // 5's 200 Mbp genome has 2e8) a third level splits every fine bucket into 2^sbits
    // fixed-capacity sub-buckets of <= 800 estimated keys in 1664-slot tables (78 KB: two
    // workgroups per CU); measured before: such inputs fell to the HBM table (k_count 130 ms of
    // a 335 ms step at 1.25e9 positions).
    if (kn().verbose)
        fprintf(stderr, "count_wpart: mb %d P %llu est %.0f lens2 %u skew %u maxlocal %u wbv_long %u\n", (int)mb,
                (unsigned long long)hsc.npos, hsc.est, hsc.lens[2], hsc.skew, hsc.maxlocal, hsc.wbv_long);
    if (mb && hsc.wbv_long) {  // reads of several lengths: hash buckets instead
        if (mb_declined) *mb_declined = true;
        return reset();
    }
    if (hsc.lens[2] || hsc.skew || hsc.maxlocal > MAX_LOCAL_EVENT || !P) return reset();
    int sbits = 0;
    // keys per third-level table: <= 800 on hash buckets; <= 400 on minimizer buckets, whose
    // tables hold whole minimizers (~25 k-mers each): config 5's 2^18 tables of mean 763 keys
    // reached 1808, past the 1664 slots (a numpy model of its genome reproduces the five
    // overflowing tables); 2^19 of mean 381 top out at 1421
    // (1024-slot tables of <= 200 keys for the run tables, two workgroups a CU, measured 3x
    // slower on config 5's shape: 355 vs 117 ms)
    const double per3 = mb ? 400.0 : 800.0;
    if (est / FINE_W > 1800.0) {
        while (sbits < 6 && est / (double)(FINE_W << sbits) > per3) sbits++;
        if (est / (double)(FINE_W << sbits) > per3) return reset();
    }
    if (kn().wide_l3 > 0) sbits = std::min(6, kn().wide_l3);
    s->stats.n_reads = nreads;
    s->stats.n_positions = P;
    s->stats.n_distinct_est = (uint64_t)llround(est);

    int bbits = 0;
    int maxb = FINE_W_BITS;  // (EULERHIP_WIDE_MAX_BBITS: tests force bucket overflow)
    if (kn().wide_max_bbits >= 0) maxb = std::max(0, std::min(FINE_W_BITS, kn().wide_max_bbits));
    if (sbits) bbits = FINE_W_BITS;
    while (bbits < maxb && est / (double)(1ull << bbits) > 1100.0) bbits++;
    int fan = 0;
    while ((1 << (fan + 1)) <= REFINE_FANOUT) fan++;
    const int cbits = std::min(bbits, std::min(DS_MAX_CBITS, std::max(1, bbits - fan)));
    const uint64_t Bk = 1ull << bbits, Ck = 1ull << cbits;
    const uint64_t Bt = Bk << sbits;  // tables
    const unsigned int SLOTS = sbits ? 1664u : (unsigned int)SLOTS_W;
    mark(s, 2 * EC_STAGE_COUNT);
    EC_CHECK(s->cnt.ensure(Ck * ngroups * 8));
    EC_CHECK(s->offs.ensure(Ck * ngroups * 8));
    EC_CHECK(s->tot.ensure((Bk + 1) * 8));
    EC_CHECK(s->bstart.ensure((Bk + 1) * 8));
    // record buffers: window records, P of them; runs: the histogram's total (hsc.nrec, exact),
    // and where the bucket pass rolls the runs out of 2-bit codes (third level) the codes go
    // into the refined runs' buffer -- ceil((windows + k - 1) / 16) dwords a run (k_run_ccount).
    // (Both buffers took P 24-B records before: 2 x 30 GB at config 5's rank shape for ~1.3 GB
    // of runs and ~2 GB of codes.)  The two-level case expands the runs into P window records.
    const size_t rbytes = runs ? sizeof(RunWM) : sizeof(RecW);
    const bool second = bbits > cbits;
    const bool direct = runs && sbits && kn().wide_runs != 2;
    const uint64_t NR = runs ? hsc.nrec : P;
    uint64_t b_recs = std::max<uint64_t>(P, 1) * sizeof(RecW), b_recs2 = b_recs;
    if (direct) {
        const uint64_t cbytes = 4 * ((P + NR * (uint64_t)(k - 1)) / 16 + 2 * NR + 64);
        b_recs = b_recs2 = std::max<uint64_t>(std::max<uint64_t>(NR, 1) * sizeof(RunWM), cbytes);
    } else if (runs) {  // the runs' input buffer rin (recs2 after a refine, else recs) takes the windows
        b_recs = std::max<uint64_t>(P, 1) * sizeof(RecW);
        b_recs2 = std::max<uint64_t>(NR, 1) * sizeof(RunWM);
        if (second) std::swap(b_recs, b_recs2);
    }
    EC_CHECK(s->recs.ensure(b_recs));
    if (second || runs) EC_CHECK(s->recs2.ensure(b_recs2));
    s->stats.record_bytes = (uint32_t)rbytes;
    s->stats.n_records = NR;
    k_coarse<FINE_W_BITS><<<grid_for(Ck * ngroups, B, 8192), B, 0, st>>>(s->hist.as<unsigned int>(), ngroups, cbits,
                                                                        s->cnt.as<unsigned long long>());
    EC_CHECK(scan_u64(s, s->cnt.as<unsigned long long>(), s->offs.as<unsigned long long>(), Ck * ngroups));
    k_bucket_totals<FINE_W_BITS><<<grid_for(Bk + 1, B), B, 0, st>>>(ftot, bbits, s->tot.as<unsigned long long>());
    EC_CHECK(scan_u64(s, s->tot.as<unsigned long long>(), s->bstart.as<unsigned long long>(), Bk + 1));
    kmark(s, 1, 0);
    if (runs)
        k_downsweep_wr<<<(unsigned)ngroups, TILE_READS, 0, st>>>(d_off, nreads, k, gsize, ngroups, cbits,
                                                                s->offs.as<unsigned long long>(), s->recs.as<RunWM>(),
                                                                wbv, mbM);
    else if (mb)
        k_downsweep_w<true><<<(unsigned)ngroups, TILE_READS, 0, st>>>(d_reads, d_off, nreads, k, gsize, ngroups, cbits,
                                                                     s->offs.as<unsigned long long>(),
                                                                     s->recs.as<RecW>(), read_base, wbv, mbM);
    else
        k_downsweep_w<false><<<(unsigned)ngroups, TILE_READS, 0, st>>>(d_reads, d_off, nreads, k, gsize, ngroups,
                                                                      cbits, s->offs.as<unsigned long long>(),
                                                                      s->recs.as<RecW>(), read_base, nullptr, 0u);
    kmark(s, 1, 1);
    if (second) {
        const unsigned RS = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(8, 1024 / Ck));
        EC_CHECK(s->gcur.ensure(Bk * 8));
        EC_HIP(hipMemcpyAsync(s->gcur.p, s->bstart.p, Bk * 8, hipMemcpyDeviceToDevice, st));
        kmark(s, 4, 0);
        if (runs)
            k_refine<RunWM, StoreRM, StoreRM><<<dim3((unsigned)Ck, RS), BUCKET_THREADS, 0, st>>>(
                StoreRM{s->recs.as<RunWM>()}, StoreRM{s->recs2.as<RunWM>()}, s->bstart.as<unsigned long long>(),
                s->gcur.as<unsigned long long>(), cbits, bbits);
        else if (mb)
            k_refine<RecWM, StoreWM, StoreWM><<<dim3((unsigned)Ck, RS), BUCKET_THREADS, 0, st>>>(
                StoreWM{s->recs.as<RecWM>()}, StoreWM{s->recs2.as<RecWM>()}, s->bstart.as<unsigned long long>(),
                s->gcur.as<unsigned long long>(), cbits, bbits);
        else
            k_refine<RecW, StoreW, StoreW><<<dim3((unsigned)Ck, RS), BUCKET_THREADS, 0, st>>>(
                StoreW{s->recs.as<RecW>()}, StoreW{s->recs2.as<RecW>()}, s->bstart.as<unsigned long long>(),
                s->gcur.as<unsigned long long>(), cbits, bbits);
        if (sbits && !runs) {  // fine buckets (recs2) -> their sub-buckets (recs), exact (k_split3)
            EC_CHECK(s->bb2.ensure((Bt + 1) * 8));
            const unsigned long long cap3 = kn().wide_l3_cap > 0 ? (unsigned long long)kn().wide_l3_cap : 0ull;
            if (mb)
                k_split3<RecWM><<<(unsigned)Bk, 512, 0, st>>>(s->recs2.as<RecWM>(), s->bstart.as<unsigned long long>(),
                                                              bbits, sbits, s->recs.as<RecWM>(),
                                                              s->bb2.as<unsigned long long>(), cap3, &dsc->overflow);
            else
                k_split3<RecW><<<(unsigned)Bk, 512, 0, st>>>(s->recs2.as<RecW>(), s->bstart.as<unsigned long long>(),
                                                             bbits, sbits, s->recs.as<RecW>(),
                                                             s->bb2.as<unsigned long long>(), cap3, &dsc->overflow);
        }
        kmark(s, 4, 1);
    }
    RecWM *rwin = nullptr;  // runs: the window records of the expansion, bucket bounds in bb2
    RunWM *rdirect = nullptr;  // runs on third-level tables: sorted runs, bounds in run units (bb2)
    uint32_t *wcodes = nullptr;  // ... and their bases as 2-bit codes, table t's from wcodes_tab[t]
    if (runs && sbits && kn().wide_runs != 2) {
        // each fine bucket's runs split into its sub-buckets (run units); the bucket pass rolls
        // the windows out itself (k_bucket_wr)
        RunWM *rin = second ? s->recs2.as<RunWM>() : s->recs.as<RunWM>();
        rdirect = second ? s->recs.as<RunWM>() : s->recs2.as<RunWM>();
        EC_CHECK(s->bb2.ensure((Bt + 1) * 8));
        const unsigned long long cap3 = kn().wide_l3_cap > 0 ? (unsigned long long)kn().wide_l3_cap : 0ull;
        kmark(s, 4, 0);
        k_split3<RunWM><<<(unsigned)Bk, 512, 0, st>>>(rin, s->bstart.as<unsigned long long>(), bbits, sbits, rdirect,
                                                      s->bb2.as<unsigned long long>(), cap3, &dsc->overflow);
        // the sorted runs' bases as 2-bit codes (the refined runs' buffer is free: P 24-B records
        // hold them -- at most 20 code dwords a run)
        EC_CHECK(s->tot.ensure((Bk + 1) * 8));
        EC_CHECK(s->gcur.ensure((Bk + 1) * 8));
        EC_CHECK(s->wcodes_tab.ensure((Bt + 1) * 8));
        k_run_ccount<<<(unsigned)(Bk + 1), 256, 0, st>>>(rdirect, s->bstart.as<unsigned long long>(), k,
                                                        s->tot.as<unsigned long long>(), Bk);
        EC_CHECK(scan_u64(s, s->tot.as<unsigned long long>(), s->gcur.as<unsigned long long>(), Bk + 1));
        wcodes = reinterpret_cast<uint32_t *>(rin);
        k_run_codes<<<(unsigned)Bk, 512, 0, st>>>(rdirect, s->bstart.as<unsigned long long>(),
                                                  s->gcur.as<unsigned long long>(), s->bb2.as<unsigned long long>(),
                                                  sbits, wcodes, s->wcodes_tab.as<unsigned long long>(),
                                                  RunReads{d_reads, d_off, k, mbM, read_base, rpack, rpack_d});
        kmark(s, 4, 1);
    } else if (runs) {
        // each fine bucket's runs sorted by sub-bucket (k_split3_runs, run units), then expanded
        // into its windows' records (k_expand_runs, window units; bb2 = sub-bucket bounds)
        RunWM *rin = second ? s->recs2.as<RunWM>() : s->recs.as<RunWM>();
        RunWM *rsorted = second ? s->recs.as<RunWM>() : s->recs2.as<RunWM>();
        rwin = reinterpret_cast<RecWM *>(rin);  // (the refined runs are dead after the sort)
        EC_CHECK(s->bb2.ensure((Bt + 1) * 8));
        EC_CHECK(s->tot.ensure((Bk + 1) * 8));
        EC_CHECK(s->gcur.ensure((Bk + 1) * 8));
        kmark(s, 4, 0);
        k_run_wsum<<<(unsigned)(Bk + 1), 256, 0, st>>>(rin, s->bstart.as<unsigned long long>(),
                                                      s->tot.as<unsigned long long>(), Bk);
        EC_CHECK(scan_u64(s, s->tot.as<unsigned long long>(), s->gcur.as<unsigned long long>(), Bk + 1));
        k_split3_runs<<<(unsigned)Bk, 512, 0, st>>>(rin, s->bstart.as<unsigned long long>(), bbits, sbits,
                                                    s->gcur.as<unsigned long long>(), rsorted,
                                                    s->bb2.as<unsigned long long>(),
                                                    sbits && kn().wide_l3_cap > 0 ? (unsigned long long)kn().wide_l3_cap
                                                                                  : 0ull,
                                                    &dsc->overflow);
        k_expand_runs<<<(unsigned)Bk, 512, 0, st>>>(rsorted, s->bstart.as<unsigned long long>(),
                                                    s->gcur.as<unsigned long long>(), rwin,
                                                    RunReads{d_reads, d_off, k, mbM, read_base});
        kmark(s, 4, 1);
    }
    mark(s, 2 * EC_STAGE_COUNT + 1);
    mark(s, 2 * EC_STAGE_COMPACT);
    const uint64_t umax = Bt * SLOTS;
    EC_CHECK(s->dkey.ensure(umax * sizeof(K128)));
    EC_CHECK(s->dcnt.ensure(umax * 4));
    EC_CHECK(s->dfc.ensure(umax * 8));
    EC_CHECK(s->dft.ensure(umax * 8));
    if (!s->no_index) EC_CHECK(s->sub.ensure(umax * sizeof(SubSlotW)));
    // minimizer buckets: each bucket's first dense id marked for the tile ranking (k_tile_plan)
    unsigned int *bm = nullptr;
    if (mb) {
        const size_t words = umax / 32 + 2;
        EC_CHECK(s->bmark.ensure(words * 4));
        EC_HIP(hipMemsetAsync(s->bmark.p, 0, words * 4, st));
        bm = s->bmark.as<unsigned int>();
    }
    kmark(s, 2, 0);
#define EC_BUCKET_W(SL, R, SRC, BEG, END)                                                                       \
    k_bucket_w<SL, R><<<(unsigned)Bt, BUCKET_THREADS, 0, st>>>(                                                  \
        SRC, BEG, END, limit, s->dkey.as<K128>(), s->dcnt.as<unsigned int>(), s->dfc.as<unsigned long long>(),    \
        s->dft.as<unsigned long long>(), s->no_index ? nullptr : s->sub.as<SubSlotW>(), &dsc->nsolid,            \
        &dsc->ndistinct, &dsc->overflow, bm)
    if (rdirect)  // (two 79-KB workgroups a CU)
        k_bucket_wr<1664, 512, 1024, LSlotW40><<<(unsigned)Bt, 512, 0, st>>>(
            rdirect, s->bb2.as<unsigned long long>(), s->bb2.as<unsigned long long>() + 1, limit, s->dkey.as<K128>(),
            s->dcnt.as<unsigned int>(), s->dfc.as<unsigned long long>(), s->dft.as<unsigned long long>(),
            s->no_index ? nullptr : s->sub.as<SubSlotW>(), &dsc->nsolid, &dsc->ndistinct, &dsc->overflow, bm,
            RunReads{d_reads, d_off, k, mbM, read_base}, wcodes, s->wcodes_tab.as<unsigned long long>());
    else if (sbits && runs)
        EC_BUCKET_W(1664, RecWM, rwin, s->bb2.as<unsigned long long>(), s->bb2.as<unsigned long long>() + 1);
    else if (runs)
        EC_BUCKET_W(SLOTS_W, RecWM, rwin, s->bb2.as<unsigned long long>(), nullptr);
    else if (sbits && mb)
        EC_BUCKET_W(1664, RecWM, s->recs.as<RecWM>(), s->bb2.as<unsigned long long>(),
                    s->bb2.as<unsigned long long>() + 1);
    else if (sbits)
        EC_BUCKET_W(1664, RecW, s->recs.as<RecW>(), s->bb2.as<unsigned long long>(),
                    s->bb2.as<unsigned long long>() + 1);
    else if (mb)
        EC_BUCKET_W(SLOTS_W, RecWM, second ? s->recs2.as<RecWM>() : s->recs.as<RecWM>(),
                    s->bstart.as<unsigned long long>(), nullptr);
    else
        EC_BUCKET_W(SLOTS_W, RecW, second ? s->recs2.as<RecW>() : s->recs.as<RecW>(), s->bstart.as<unsigned long long>(),
                    nullptr);
#undef EC_BUCKET_W
    kmark(s, 2, 1);
    mark(s, 2 * EC_STAGE_COMPACT + 1);
    unsigned long long nruns = 0;
    if (runs) EC_CHECK(d2h(s, &nruns, s->bstart.as<unsigned long long>() + Bk, 8, st));
    EC_CHECK(d2h(s, &hsc, dsc, sizeof(Scalars), st));
    EC_CHECK(host_sync(s, st));
    if (runs) s->stats.n_records = nruns;
    if (hsc.overflow) {  // a bucket outgrew its LDS table: the caller counts on the HBM table
        if (kn().verbose)
            fprintf(stderr, "count_wpart: %u tables overflowed (%llu tables of %u slots, sbits %d, mb %d)\n",
                    hsc.overflow, (unsigned long long)Bt, SLOTS, sbits, (int)mb);
        s->stats.table_retries++;
        return reset();
    }
    U = hsc.nsolid;
    s->stats.n_distinct = hsc.ndistinct;
    s->stats.n_solid = U;
    s->stats.count_path = EC_PATH_PARTITIONED;
    s->stats.n_buckets = (uint32_t)Bt;
    s->stats.table_capacity = umax;
    sidx.table = nullptr;
    sidx.capmask = 0;
    sidx.sub = s->sub.as<SubSlotW>();
    sidx.bbits = bbits + sbits;
    sidx.slots = SLOTS;
    sidx.mb = mb ? 1 : 0;
    sidx.k = k;
    EC_CHECK(check_node_ids(U));
    s->bmark_ok = bm != nullptr;
    ok = true;
    return EC_OK;
}

int phase_count_w(ec_session *s, const uint8_t *d_reads, const uint64_t *d_off, uint64_t nreads, uint64_t read_base,
                  int k, long long limit, unsigned int &U, SolidIndexW &sidx) {
    if (nreads + read_base > (1ull << 32)) {
        set_error("global read ids reach %llu >= 2^32", (unsigned long long)(nreads + read_base));
        return EC_ERR_ARG;
    }
    bool ok = false;
    {
        // minimizer buckets for k <= 52 (count_wide.h; EULERHIP_WIDE_MB=0: hash buckets)
        bool declined = false;
        // (config-5 rank shape: 141 ms a step against 169 ms on mix128 buckets --
        // profiles/r04_l_config5_rank_shape_minimizer_buckets.json)
        const bool mb = k <= WMB_MAX_K && kn().wide_mb != 0;
        EC_CHECK(phase_count_wpart(s, d_reads, d_off, nreads, read_base, k, limit, U, sidx, ok, mb, &declined));
        if (declined) EC_CHECK(phase_count_wpart(s, d_reads, d_off, nreads, read_base, k, limit, U, sidx, ok));
    }
    if (ok) return EC_OK;
    s->stats.n_reads = nreads;
    hipStream_t st = s->stream;
    const unsigned B = 256;
    Scalars *dsc = s->scal.as<Scalars>();
    Scalars hsc;
    mark(s, 2 * EC_STAGE_PRESCAN);
    EC_CHECK(s->hll.ensure(HLL_M * 4));
    EC_HIP(hipMemsetAsync(s->hll.p, 0, HLL_M * 4, st));
    if (nreads) {
        k_prescan_w<<<grid_for(nreads, B, 4096), B, 0, st>>>(d_reads, d_off, nreads, k, s->hll.as<unsigned int>(),
                                                            &dsc->npos, &dsc->bad);
        k_hll_final<<<1, 1024, 0, st>>>(s->hll.as<unsigned int>(), HLL_BITS, &dsc->est);
    }
    mark(s, 2 * EC_STAGE_PRESCAN + 1);
    EC_CHECK(d2h(s, &hsc, dsc, sizeof(Scalars), st));
    EC_CHECK(host_sync(s, st));
    EC_CHECK(check_alphabet(d_reads, hsc.bad));
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
            k_count_w<<<grid_for(nreads, B), B, 0, st>>>(d_reads, d_off, nreads, k, s->table.as<SlotW>(), cap - 1,
                                                        &dsc->overflow, read_base);
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
    return finish_wide(s, cap, limit, U, sidx);
}

// The owner merge's dense set (U ids in table order) reordered by minimizer (shard.h k_wplace /
// k_wpermute), the minimizers' first ids marked for the partitioned finish's tiles: the
// gathered ids of 128-bit keys get the locality minimizer owners give (round 5)
int order_by_minimizer_w(ec_session *s, unsigned int U) {
    hipStream_t st = s->stream;
    const unsigned B = 256;
    if (!U) return EC_OK;
    EC_CHECK(s->skeys.ensure((size_t)U * 8));
    EC_CHECK(s->skeys2.ensure((size_t)U * 8));
    EC_CHECK(s->svals.ensure((size_t)U * 4));
    EC_CHECK(s->svals2.ensure((size_t)U * 4));
    k_wplace<<<grid_for(U, B), B, 0, st>>>(s->dkey.as<K128>(), U, s->k, s->skeys.as<unsigned long long>(),
                                           s->svals.as<unsigned int>());
    EC_CHECK(sort_pairs(s, s->skeys.as<unsigned long long>(), s->skeys2.as<unsigned long long>(),
                        s->svals.as<unsigned int>(), s->svals2.as<unsigned int>(), U));
    // permuted into the count-phase record buffers (free on the owner side), then swapped in
    EC_CHECK(s->recs.ensure((size_t)U * sizeof(K128)));
    EC_CHECK(s->recs2.ensure((size_t)U * 16));
    EC_CHECK(s->mbid2.ensure((size_t)U * 4));
    unsigned long long *nfc = s->recs2.as<unsigned long long>(), *nft = nfc + U;
    k_wpermute<<<grid_for(U, B), B, 0, st>>>(s->svals2.as<unsigned int>(), U, s->dkey.as<K128>(),
                                             s->dcnt.as<unsigned int>(), s->dfc.as<unsigned long long>(),
                                             s->dft.as<unsigned long long>(), s->recs.as<K128>(),
                                             s->mbid2.as<unsigned int>(), nfc, nft);
    std::swap(s->dkey, s->recs);
    std::swap(s->dcnt, s->mbid2);
    EC_CHECK(s->dfc.ensure((size_t)U * 8));
    EC_CHECK(s->dft.ensure((size_t)U * 8));
    EC_HIP(hipMemcpyAsync(s->dfc.p, nfc, (size_t)U * 8, hipMemcpyDeviceToDevice, st));
    EC_HIP(hipMemcpyAsync(s->dft.p, nft, (size_t)U * 8, hipMemcpyDeviceToDevice, st));
    const unsigned int words = U / 32 + 2;
    EC_CHECK(s->bmark.ensure((size_t)words * 4));
    k_wmarks<<<grid_for(words, B), B, 0, st>>>(s->skeys2.as<unsigned long long>(), U, s->bmark.as<unsigned int>(), words);
    s->seg_marks = U;
    return EC_OK;
}

int phase_merge_w(ec_session *s, const AggW *d_agg, uint64_t n, long long limit, unsigned int &U, SolidIndexW &sidx) {
    hipStream_t st = s->stream;
    const unsigned B = 256;
    Scalars *dsc = s->scal.as<Scalars>();
    Scalars hsc;
    // the table for the distinct keys (HyperLogLog of the records' keys, +-2.3 %), not for the
    // records: a rank's merge sees each key once per source (a table past 0.45 load retries x4)
    double keys = (double)n;
    if (n >= (1u << 20)) {
        constexpr int HB = HLL_REG_BITS;
        EC_CHECK(s->ftot.ensure((1 << HB) * 4));
        unsigned int *hreg = s->ftot.as<unsigned int>();
        EC_HIP(hipMemsetAsync(hreg, 0, (1 << HB) * 4, st));
        k_hll_aggw<<<256, B, 0, st>>>(d_agg, n, HB, hreg);
        k_hll_final<<<1, 1024, 0, st>>>(hreg, HB, &dsc->est);
        double est = 0;
        EC_CHECK(d2h(s, &est, &dsc->est, sizeof(double), st));
        EC_CHECK(host_sync(s, st));
        keys = std::min((double)n, est * 1.1 + 1024.0);
    }
    uint64_t cap = 1024;
    while (cap < (uint64_t)(2.2 * keys) + 1024) cap <<= 1;
    for (int attempt = 0;; attempt++) {
        EC_CHECK(s->table.ensure(cap * sizeof(SlotW)));
        mark(s, 2 * EC_STAGE_COUNT);
        k_table_clear_w<<<grid_for(cap, B, 8192), B, 0, st>>>(s->table.as<SlotW>(), cap);
        EC_HIP(hipMemsetAsync(&dsc->overflow, 0, 4, st));
        if (n) k_merge_agg_w<<<grid_for(n, B), B, 0, st>>>(d_agg, n, s->table.as<SlotW>(), cap - 1, &dsc->overflow);
        mark(s, 2 * EC_STAGE_COUNT + 1);
        EC_CHECK(d2h(s, &hsc.overflow, &dsc->overflow, 4, st));
        EC_CHECK(host_sync(s, st));
        if (!hsc.overflow) break;
        if (attempt >= 4) {
            set_error("merge table overflow at capacity %llu", (unsigned long long)cap);
            return EC_ERR_CAPACITY;
        }
        cap <<= 2;
        s->stats.table_retries++;
    }
    EC_CHECK(finish_wide(s, cap, limit, U, sidx, std::max<uint64_t>(n, 1)));
    // an owner merge (no lookup index wanted) on minimizer owners: ids in minimizer order
    if (s->no_index && s->owner_rule == 0 && merge_wmb(s->k) && !(s->flags & EC_FLAG_GENERAL)) {
        EC_CHECK(order_by_minimizer_w(s, U));
        sidx.table = nullptr;  // (the table's ids are the pre-order ones)
    }
    return EC_OK;
}

}  // namespace
