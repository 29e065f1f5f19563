// dense_filter.h -- the held dense records re-filtered by a new solid limit, in their order
// (ec_dense_refilter; include/eulerhip.h): the sharded path's counterpart of ec_refilter.
//
// After ec_count_shard / ec_merge_owned* a session holds its records as four parallel arrays
// dkey (8 B, or K128 16 B for k > 32), dcnt (4 B), dfc, dft (8 B each), [0 .. n).  The filter keeps
// the records with dcnt > limit and closes the gaps: an order-preserving compaction of the four
// arrays by one predicate, shaped like compact.h -- per-span counts, one scan, a write pass that
// ranks the kept records of a span by wave ballots; no contended global counter.
//   k_dense_count  kept records of each span of DF_SPAN (bc[span]), and the removed total into the
//                  call's only read-back: a lane counts its own, a wave sums by shuffles, one
//                  global atomic per workgroup.  A zero total ends the call before any write.
//   k_dense_write  bs = inclusive scan of bc.  A workgroup walks its span DF_STEP records at a
//                  time; every thread takes four consecutive counts with one 16-B load (as
//                  k_spectrum / k_refilter_mark), so the record order is thread-major: a thread's
//                  first output slot is the span's base + the kept records of the steps before +
//                  those of the lower waves (LDS) + those of the lower lanes (four ballots, one
//                  per quad position) -- then its own kept records in quad order.  Keys and first
//                  events are loaded only where the quad keeps something (8-B arrays as 16-B
//                  pairs, a 16-B key on its own) and stored record by record: a wave's stores
//                  of one array fall into one window of at most 256 consecutive records.
//
// Not in place.  A span's output range lies at or below its own input, so it can cover the input
// of a lower span whose workgroup has not read it yet; the write pass therefore compacts into
// session scratch -- recs (keys), midx (counts), recs2 (the two event arrays): the buffers
// ec_graph_place stages the same four arrays in, free wherever the dense records are valid, since
// every call that leaves them valid is done with its own use of that scratch -- and the kept
// prefix is copied back on the stream (device to device, 28 / 36 B per kept record read and
// written once more).  Exchanging the buffers instead would save that copy, but dfc and dft are
// two allocations and the event scratch is one, and every holder of a dense-array pointer or
// capacity (bucket marks, the speculated prologues' shapes) would have to follow the exchange;
// the copy keeps the four arrays where everything else expects them.  The predicate is read from
// dcnt in both passes, and dcnt is not written before the copy back, which the stream orders
// behind the write pass.
#pragma once
#include "compact.h"
#include "spectrum.h"

namespace ec {

constexpr unsigned int DF_SPAN = COMPACT_CHUNK;  // records per workgroup
constexpr unsigned int DF_STEP = 4 * 256;        // records per workgroup step: a quad per thread
static_assert(DF_SPAN % DF_STEP == 0, "a span is whole steps: every quad of a span is 16-B aligned");

// the counts of the quad at u0 (a multiple of 4) of the span ending at c1, and which of them are
// kept (bit j: record u0 + j exists and has count > limit); dcnt is the start of a device allocation
__device__ inline unsigned int df_quad(const unsigned int *dcnt, uint64_t u0, uint64_t c1, unsigned int limit,
                                       uint4 &c) {
    c = make_uint4(0u, 0u, 0u, 0u);
    if (u0 + 4 <= c1) {
        c = *reinterpret_cast<const uint4 *>(dcnt + u0);
    } else {
        if (u0 < c1) c.x = dcnt[u0];
        if (u0 + 1 < c1) c.y = dcnt[u0 + 1];
        if (u0 + 2 < c1) c.z = dcnt[u0 + 2];
    }
    // (a record past c1 reads as count 0: kept only if it exists)
    return (unsigned int)(u0 < c1 && c.x > limit) | (unsigned int)(u0 + 1 < c1 && c.y > limit) << 1 |
           (unsigned int)(u0 + 2 < c1 && c.z > limit) << 2 | (unsigned int)(u0 + 3 < c1 && c.w > limit) << 3;
}

__global__ void __launch_bounds__(256) k_dense_count(const unsigned int *dcnt, unsigned int n, unsigned int limit,
                                                     unsigned int *bc, RefilterTotals *tot) {
    __shared__ unsigned int wsum[4];
    const uint64_t c0 = (uint64_t)blockIdx.x * DF_SPAN;
    const uint64_t c1 = c0 + DF_SPAN < n ? c0 + DF_SPAN : n;
    unsigned int kept = 0;
    for (uint64_t u0 = c0 + 4 * threadIdx.x; u0 < c1; u0 += DF_STEP) {
        uint4 c;
        kept += __popc(df_quad(dcnt, u0, c1, limit, c));
    }
    for (int d = 32; d; d >>= 1) kept += __shfl_xor(kept, d);  // (the whole wave is here: the loop has ended)
    if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = kept;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned int v = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        bc[blockIdx.x] = v;
        const unsigned long long removed = (c1 - c0) - v;
        if (removed) atomicAdd(&tot->n_removed, removed);
    }
}

// the kept records of a quad: 8-B values as two 16-B pairs where the quad is whole (32-B aligned)
__device__ inline void df_load4(const unsigned long long *p, uint64_t u0, unsigned int keep, bool whole,
                                unsigned long long v[4]) {
    if (whole) {
        if (keep & 3u) {
            const ulonglong2 a = *reinterpret_cast<const ulonglong2 *>(p + u0);
            v[0] = a.x, v[1] = a.y;
        }
        if (keep & 12u) {
            const ulonglong2 b = *reinterpret_cast<const ulonglong2 *>(p + u0 + 2);
            v[2] = b.x, v[3] = b.y;
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (keep >> j & 1u) v[j] = p[u0 + j];
}

// bs = inclusive scan of the span counts; the outputs hold bs[last] records
template <typename KeyT>
__global__ void __launch_bounds__(256) k_dense_write(const KeyT *dkey, const unsigned int *dcnt,
                                                     const unsigned long long *dfc, const unsigned long long *dft,
                                                     unsigned int n, unsigned int limit, const unsigned int *bs,
                                                     KeyT *okey, unsigned int *ocnt, unsigned long long *ofc,
                                                     unsigned long long *oft) {
    __shared__ unsigned int wsum[4];
    const uint64_t c0 = (uint64_t)blockIdx.x * DF_SPAN;
    const uint64_t c1 = c0 + DF_SPAN < n ? c0 + DF_SPAN : n;
    unsigned int base = blockIdx.x ? bs[blockIdx.x - 1] : 0u;
    if (bs[blockIdx.x] == base) return;  // (uniform: the span keeps nothing)
    const unsigned int lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1;
    for (uint64_t i0 = c0; i0 < c1; i0 += DF_STEP) {
        const uint64_t u0 = i0 + 4 * threadIdx.x;
        uint4 c;
        const unsigned int keep = df_quad(dcnt, u0, c1, limit, c);
        const unsigned long long m0 = __ballot(keep & 1u), m1 = __ballot(keep & 2u), m2 = __ballot(keep & 4u),
                                 m3 = __ballot(keep & 8u);
        if (lane == 0) wsum[wid] = (unsigned int)(__popcll(m0) + __popcll(m1) + __popcll(m2) + __popcll(m3));
        __syncthreads();
        unsigned int o = base;
        for (unsigned int q = 0; q < wid; q++) o += wsum[q];
        const unsigned int tot = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (keep) {
            o += (unsigned int)(__popcll(m0 & below) + __popcll(m1 & below) + __popcll(m2 & below) +
                                __popcll(m3 & below));
            const bool whole = u0 + 4 <= c1;
            unsigned long long key[4], fc[4], ft[4];
            if constexpr (sizeof(KeyT) == 8) df_load4(dkey, u0, keep, whole, key);
            df_load4(dfc, u0, keep, whole, fc);
            df_load4(dft, u0, keep, whole, ft);
            const unsigned int cc[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (keep >> j & 1u) {
                    if constexpr (sizeof(KeyT) == 8) okey[o] = key[j];
                    else okey[o] = dkey[u0 + j];  // (a 16-B key goes straight through: one load, one store)
                    ocnt[o] = cc[j];
                    ofc[o] = fc[j];
                    oft[o] = ft[j];
                    o++;
                }
        }
        base += tot;
        __syncthreads();
    }
}

}  // namespace ec
