// spectrum.h -- the k-mer count spectrum of the session's dict and the re-filter by a new solid
// limit (ec_kmer_spectrum, ec_refilter; include/eulerhip.h).
//
// Both read only the dense dict counts dcnt[0 .. U) a one-GPU graph phase leaves on the device (one
// u32 per canonical solid k-mer: its dict count).  Every thread takes four consecutive counts with
// one 16-B load; the last quad of a U that is no multiple of 4 is read count by count.
//   k_spectrum       hist[min(count, nbins - 1)] += 1.  A workgroup counts into LDS first -- one
//                    histogram per wave while four of them fit SPEC_LDS_BINS (nbins <= 1024), one
//                    for the workgroup above that -- and adds its non-zero bins to the global
//                    histogram with one 64-bit atomic each.  A deep-coverage dict puts most counts
//                    into the ~30 bins around the coverage peak, so a wave's LDS atomics meet on
//                    few addresses; the per-wave copies keep the four waves off each other's.
//   k_refilter_mark  killed[u] = (count <= limit), and the number of marked ids into the round's
//                    totals record: a lane counts its own, a wave sums them by shuffles, and one
//                    global atomic per workgroup adds the four waves' sums.  k_clip_export
//                    (clip.h) then writes the marked ids as filler records, as a clipping round.
#pragma once
#include "common.h"

namespace ec {

constexpr unsigned int SPEC_LDS_BINS = 4096;  // u32 bins a workgroup holds in LDS (16 KB)

struct RefilterTotals {  // the re-filter round's only read-back
    unsigned long long n_removed;  // canonical k-mers with count <= limit
    unsigned long long pad;
};

// dcnt is the start of a device allocation (16-B aligned); nbins <= SPEC_LDS_BINS
__global__ void __launch_bounds__(256) k_spectrum(const unsigned int *dcnt, unsigned int U, unsigned int nbins,
                                                  unsigned long long *hist) {
    __shared__ unsigned int lh[SPEC_LDS_BINS];
    const unsigned int copies = 4 * nbins <= SPEC_LDS_BINS ? 4u : 1u;
    for (unsigned int b = threadIdx.x; b < copies * nbins; b += blockDim.x) lh[b] = 0;
    __syncthreads();
    unsigned int *mine = lh + (copies == 4 ? (threadIdx.x >> 6) * nbins : 0u);
    const unsigned int top = nbins - 1;
    const unsigned int nquad = (U + 3) / 4;  // (2 U < 2^31 node ids: no wrap)
    for (uint64_t q = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; q < nquad; q += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t u0 = 4 * q;
        if (u0 + 4 <= U) {
            const uint4 c = *reinterpret_cast<const uint4 *>(dcnt + u0);
            atomicAdd(&mine[min(c.x, top)], 1u);
            atomicAdd(&mine[min(c.y, top)], 1u);
            atomicAdd(&mine[min(c.z, top)], 1u);
            atomicAdd(&mine[min(c.w, top)], 1u);
        } else {
            for (uint64_t u = u0; u < U; u++) atomicAdd(&mine[min(dcnt[u], top)], 1u);
        }
    }
    __syncthreads();
    for (unsigned int b = threadIdx.x; b < nbins; b += blockDim.x) {
        unsigned long long v = lh[b];
        if (copies == 4) v += (unsigned long long)lh[nbins + b] + lh[2 * nbins + b] + lh[3 * nbins + b];
        if (v) atomicAdd(&hist[b], v);
    }
}

// killed holds U bytes at the start of a device allocation (4-B aligned quads)
__global__ void __launch_bounds__(256) k_refilter_mark(const unsigned int *dcnt, unsigned int U, unsigned int limit,
                                                       uint8_t *killed, RefilterTotals *tot) {
    __shared__ unsigned int wsum[4];
    unsigned int n = 0;  // this lane's marked ids
    const unsigned int nquad = (U + 3) / 4;
    for (uint64_t q = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; q < nquad; q += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t u0 = 4 * q;
        if (u0 + 4 <= U) {
            const uint4 c = *reinterpret_cast<const uint4 *>(dcnt + u0);
            const unsigned int k0 = c.x <= limit, k1 = c.y <= limit, k2 = c.z <= limit, k3 = c.w <= limit;
            *reinterpret_cast<unsigned int *>(killed + u0) = k0 | (k1 << 8) | (k2 << 16) | (k3 << 24);
            n += k0 + k1 + k2 + k3;
        } else {
            for (uint64_t u = u0; u < U; u++) {
                const unsigned int kk = dcnt[u] <= limit;
                killed[u] = (uint8_t)kk;
                n += kk;
            }
        }
    }
    for (int d = 32; d; d >>= 1) n += __shfl_xor(n, d);  // (the whole wave is here: the loop has ended)
    if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long v = (unsigned long long)wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (v) atomicAdd(&tot->n_removed, v);
    }
}

}  // namespace ec
