// clip.h -- tip clipping on the session's results (ec_clip_tips, include/eulerhip.h).
//
// The rule reads only what a one-GPU graph phase leaves on the device: the contig offsets
// (lengths), the GFA link table lk (8 slots a side, entry 2 j + (orientation == '-')) with its
// per-side counts lcnt, and the contig characters.  With len_i the characters of contig i:
//   candidate   len_i <= max_tip_len and exactly one side of i has links (side a);
//   siblings    per link (j, o) of side a: the contigs on j's side t (t = 1 if o == '+', the link
//               entered j at its head; else 0) other than i;
//   clipped     some sibling is no candidate, or longer, or as long with a smaller index.
// It depends on (links, lengths, indices) alone, so one thread a contig decides without order
// effects: k_clip_cand, then k_clip_pick (the clipped contigs into a compact list, their count
// and k-mer windows into two totals -- the round's only read-back).  k_clip_kill marks the dense
// id of every window of a clipped contig (one wave a contig), k_clip_export writes the dense
// arrays as exchange records with the marked ones as filler records, which the merge skips; the
// host loop (assemble.hip clip_tips) then runs the merge and the graph phase on them again.
#pragma once
#include "graph.h"
#include "shard.h"

namespace ec {

struct ClipTotals {
    unsigned int n_clip;        // contigs in the list
    unsigned int pad;
    unsigned long long n_kmer;  // their windows: sum of len - k + 1
};

__global__ void __launch_bounds__(256) k_clip_cand(const unsigned long long *coff, const unsigned int *lcnt,
                                                   unsigned int nc, unsigned long long max_len, uint8_t *cand) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < nc; i += (uint64_t)gridDim.x * blockDim.x) {
        const unsigned long long len = coff[i + 1] - coff[i];
        const bool e0 = lcnt[2 * i] == 0, e1 = lcnt[2 * i + 1] == 0;
        cand[i] = (len <= max_len && e0 != e1) ? 1 : 0;
    }
}

__global__ void __launch_bounds__(256) k_clip_pick(const unsigned long long *coff, const long long *lk,
                                                   const unsigned int *lcnt, const uint8_t *cand, unsigned int nc,
                                                   int k, unsigned int *list, ClipTotals *tot) {
    for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < nc; t += (uint64_t)gridDim.x * blockDim.x) {
        const unsigned int i = (unsigned int)t;
        if (!cand[i]) continue;
        const unsigned long long len = coff[i + 1] - coff[i];
        const unsigned int a = lcnt[2 * i] ? 0u : 1u;
        const unsigned int na = min(lcnt[2 * i + a], 8u);
        bool clip = false;
        for (unsigned int u = 0; u < na; u++) {
            const unsigned long long e = (unsigned long long)lk[(2ull * i + a) * 8 + u];
            const unsigned int j = (unsigned int)(e >> 1);
            if (j >= nc) continue;
            const unsigned int side = (e & 1) ? 0u : 1u;  // '+': entered j at its head -> its head side
            const unsigned int nj = min(lcnt[2 * j + side], 8u);
            for (unsigned int v = 0; v < nj; v++) {
                const unsigned int i2 = (unsigned int)((unsigned long long)lk[(2ull * j + side) * 8 + v] >> 1);
                if (i2 == i || i2 >= nc) continue;
                const unsigned long long len2 = coff[i2 + 1] - coff[i2];
                clip |= !cand[i2] || len2 > len || (len2 == len && i2 < i);
            }
        }
        if (clip) {
            list[atomicAdd(&tot->n_clip, 1u)] = i;  // (at most nc entries: one a contig)
            atomicAdd(&tot->n_kmer, len - (unsigned long long)k + 1);
        }
    }
}

// one wave64 a clipped contig, lanes striding its windows (a default tip has <= k + 1 <= 64)
template <typename Ops, typename Index>
__global__ void __launch_bounds__(256) k_clip_kill(Index idx, const unsigned int *list, unsigned int n_clip,
                                                   const unsigned long long *coff, const char *chars, int k,
                                                   unsigned int U, uint8_t *killed) {
    using K = typename Ops::K;
    const K mask = Ops::mask(k);
    const unsigned int lane = threadIdx.x & 63u, wpb = blockDim.x >> 6;
    for (uint64_t w = blockIdx.x * (uint64_t)wpb + (threadIdx.x >> 6); w < n_clip; w += (uint64_t)gridDim.x * wpb) {
        const unsigned int i = list[w];
        const unsigned long long lo = coff[i], len = coff[i + 1] - lo;
        if (len < (unsigned long long)k) continue;
        const unsigned long long nwin = len - (unsigned long long)k + 1;
        for (unsigned long long p = lane; p < nwin; p += 64) {
            K code{};
            for (int t = 0; t < k; t++)
                code = Ops::push(code, base_code((unsigned char)chars[lo + p + t]) & 3u, mask);
            const K tw = Ops::twin(code, k);
            const unsigned int u = idx.find(code < tw ? code : tw);
            if (u < U) killed[u] = 1;
        }
    }
}

// k_export_dense with the killed ids as filler records (all-ones key: skipped by every merge)
template <typename K> __device__ inline K clip_filler_key();
template <> __device__ inline unsigned long long clip_filler_key<unsigned long long>() { return EMPTY_KEY; }
template <> __device__ inline K128 clip_filler_key<K128>() {
    K128 f;
    f.lo = ~0ull;
    f.hi = ~0ull;
    return f;
}
template <typename K>
__global__ void __launch_bounds__(256) k_clip_export(const K *dkey, const unsigned int *dcnt,
                                                     const unsigned long long *dfc, const unsigned long long *dft,
                                                     const uint8_t *killed, unsigned int n,
                                                     typename RecOf<K>::T *out) {
    for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < n; t += (uint64_t)gridDim.x * blockDim.x)
        out[t] = killed[t] ? RecOf<K>::make(clip_filler_key<K>(), 0u, NONE64, NONE64)
                           : RecOf<K>::make(dkey[t], dcnt[t], dfc[t], dft[t]);
}

}  // namespace ec
