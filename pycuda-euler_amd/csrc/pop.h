// pop.h -- bubble popping on the session's results (ec_pop_bubbles, include/eulerhip.h) and the
// per-contig k-mer count sums it decides by (ec_copy_contig_kmer_sums).
//
// Like clip.h the rule reads what a one-GPU graph phase leaves on the device -- contig offsets,
// the link table lk (8 slots a side, entry 2 j + (orientation == '-')) with its counts lcnt, the
// contig characters -- and one thing more, the dense counts dcnt through the lookup index.  With
// len_i the characters of contig i, W_i = len_i - k + 1 and S_i the sum of the dict counts of its
// W_i windows:
//   port      a link (j, o) reaches the port 2 j + t, t = 1 if o == '+' else 0 (= entry ^ 1);
//   branch    len_i <= max_bubble_len, one link on each side, the two ports differ and neither is
//             on i itself; its key is the sorted port pair in one 64-bit word;
//   partner   another branch with the same key -- it is linked to both ports, so it is among the
//             <= 8 entries of the link side the first port names;
//   popped    some partner has S_i2 W_i > S_i W_i2, or equality there and i2 < i.
// It depends on (links, lengths, counts, indices) alone: k_pop_cand, k_contig_ksum on the
// branches, k_pop_pick (the popped contigs into clip.h's compact list and totals), and the round
// is clip.h's: kill, export with fillers, merge, graph phase.
//
// k_contig_ksum serves a million contigs of <= 2 k characters and a handful of Mbp-long ones
// alike: the work is cut into tiles of at most KSUM_TILE windows of ONE contig (tile counts per
// contig, a scan, k_ksum_tiles writes the tile -> contig table), a wave a tile.  A lane takes a
// contiguous run of ceil(n / 64) windows and rolls its code along it: k pushes for the first
// window, one for every further one.  The wave's sum goes through shuffles, the workgroup's waves
// of one contig are added in LDS, and the first of them does one 64-bit atomicAdd -- integer
// sums, exact in any order.
#pragma once
#include "clip.h"

namespace ec {

constexpr unsigned int KSUM_TILE = 1024;  // windows a tile at most: 16 a lane
constexpr unsigned long long POP_NONE = ~0ull;

// tiles of contig i: ceil(W_i / KSUM_TILE); 0 where sel (if given) holds POP_NONE for it
__global__ void __launch_bounds__(256) k_ksum_count(const unsigned long long *coff, unsigned int nc, int k,
                                                    const unsigned long long *sel, unsigned int *tcnt) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < nc; i += (uint64_t)gridDim.x * blockDim.x) {
        const unsigned long long len = coff[i + 1] - coff[i];
        const bool on = len >= (unsigned long long)k && (!sel || sel[i] != POP_NONE);
        tcnt[i] = on ? (unsigned int)((len - (unsigned long long)k + KSUM_TILE) / KSUM_TILE) : 0u;
    }
}

// the tile -> contig table: toff = exclusive scan of tcnt.  A wave a contig (a Mbp-long contig
// has thousands of tiles, a short one exactly one)
__global__ void __launch_bounds__(256) k_ksum_tiles(const unsigned int *tcnt, const unsigned int *toff,
                                                    unsigned int nc, unsigned int ntiles, unsigned int *tile_contig) {
    const unsigned int lane = threadIdx.x & 63u, wpb = blockDim.x >> 6;
    for (uint64_t i = blockIdx.x * (uint64_t)wpb + (threadIdx.x >> 6); i < nc; i += (uint64_t)gridDim.x * wpb) {
        const unsigned int n = tcnt[i], o = toff[i];
        for (unsigned int t = lane; t < n; t += 64)
            if (o + t < ntiles) tile_contig[o + t] = (unsigned int)i;
    }
}

template <typename Ops, typename Index>
__global__ void __launch_bounds__(256) k_contig_ksum(Index idx, const unsigned int *tile_contig,
                                                     const unsigned int *toff, unsigned int ntiles,
                                                     unsigned int nc, const unsigned long long *coff,
                                                     const char *chars, const unsigned int *dcnt, int k,
                                                     unsigned int U, unsigned long long *sums) {
    using K = typename Ops::K;
    __shared__ unsigned int s_c[4];
    __shared__ unsigned long long s_v[4];
    const K mask = Ops::mask(k);
    const unsigned int lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    // (blockDim.x == 256: four tiles a workgroup; every wave reaches the barrier)
    const uint64_t tile = blockIdx.x * 4ull + wv;
    unsigned int ci = NONE32;
    unsigned long long acc = 0;
    if (tile < ntiles) {
        ci = tile_contig[tile];
        if (ci < nc) {
            const unsigned long long lo = coff[ci], nwin = coff[ci + 1] - lo - (unsigned long long)k + 1;
            const unsigned long long w0 = (unsigned long long)((unsigned int)tile - toff[ci]) * KSUM_TILE;
            const unsigned int n = (unsigned int)min((unsigned long long)KSUM_TILE, nwin - w0);  // 1 .. KSUM_TILE
            const unsigned int run = (n + 63u) >> 6;                                              // windows a lane
            const unsigned int b = lane * run, e = min(b + run, n);
            if (b < e) {
                const char *p = chars + lo + w0 + b;  // reads up to p[e - b + k - 2] < coff[ci + 1]
                K code{};
                for (int t = 0; t < k - 1; t++) code = Ops::push(code, base_code((unsigned char)p[t]) & 3u, mask);
                for (unsigned int w = 0; w < e - b; w++) {
                    code = Ops::push(code, base_code((unsigned char)p[k - 1 + w]) & 3u, mask);
                    const K tw = Ops::twin(code, k);
                    const unsigned int u = idx.find(code < tw ? code : tw);
                    if (u < U) acc += dcnt[u];
                }
            }
        } else {
            ci = NONE32;
        }
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o);
    if (lane == 0) {
        s_c[wv] = ci;
        s_v[wv] = acc;
    }
    __syncthreads();
    // the first wave of each run of equal contigs adds the run (tiles of one contig are adjacent)
    if (lane == 0 && ci != NONE32 && (wv == 0 || s_c[wv - 1] != ci)) {
        unsigned long long v = acc;
        for (unsigned int w = wv + 1; w < 4 && s_c[w] == ci; w++) v += s_v[w];
        atomicAdd(&sums[ci], v);
    }
}

// the branch test, a thread a contig: the sorted port pair as one key, or POP_NONE
__global__ void __launch_bounds__(256) k_pop_cand(const unsigned long long *coff, const long long *lk,
                                                  const unsigned int *lcnt, unsigned int nc,
                                                  unsigned long long max_len, unsigned long long *key) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < nc; i += (uint64_t)gridDim.x * blockDim.x) {
        unsigned long long q = POP_NONE;
        if (coff[i + 1] - coff[i] <= max_len && lcnt[2 * i] == 1 && lcnt[2 * i + 1] == 1) {
            const unsigned long long p0 = (unsigned long long)lk[(2 * i) * 8] ^ 1ull;
            const unsigned long long p1 = (unsigned long long)lk[(2 * i + 1) * 8] ^ 1ull;
            if (p0 != p1 && (p0 >> 1) != i && (p1 >> 1) != i && (p0 >> 1) < nc && (p1 >> 1) < nc)
                q = p0 < p1 ? (p0 << 32) | p1 : (p1 << 32) | p0;  // (ports < 2 nc <= 2^32)
        }
        key[i] = q;
    }
}

// a thread a branch: its partners are among the entries of the link side its smaller port names
__global__ void __launch_bounds__(256) k_pop_pick(const unsigned long long *coff, const long long *lk,
                                                  const unsigned int *lcnt, const unsigned long long *key,
                                                  const unsigned long long *sums, unsigned int nc, int k,
                                                  unsigned int *list, ClipTotals *tot) {
    for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < nc; t += (uint64_t)gridDim.x * blockDim.x) {
        const unsigned int i = (unsigned int)t;
        const unsigned long long q = key[i];
        if (q == POP_NONE) continue;
        const unsigned long long W = coff[i + 1] - coff[i] - (unsigned long long)k + 1, S = sums[i];
        const unsigned long long port = q >> 32;  // 2 j + t: side t of contig j
        const unsigned int n = min(lcnt[port], 8u);
        bool pop = false;
        for (unsigned int v = 0; v < n; v++) {
            const unsigned int i2 = (unsigned int)((unsigned long long)lk[port * 8 + v] >> 1);
            if (i2 == i || i2 >= nc || key[i2] != q) continue;
            const unsigned long long W2 = coff[i2 + 1] - coff[i2] - (unsigned long long)k + 1;
            const unsigned long long a = sums[i2] * W, b = S * W2;  // < 2^64: S < 2^32 W, W < 2^16
            pop |= a > b || (a == b && i2 < i);
        }
        if (pop) {
            list[atomicAdd(&tot->n_clip, 1u)] = i;  // (at most nc entries: one a contig)
            atomicAdd(&tot->n_kmer, W);
        }
    }
}

}  // namespace ec
