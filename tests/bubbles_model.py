"""CPU statement (test infrastructure, pure Python, small cases only) of the bubble-popping
contract that ec_pop_bubbles / Session.pop_bubbles / assembler.pop_bubbles implement on the
device, and of the per-contig k-mer count sums of ec_copy_contig_kmer_sums.

Built on model_parallel.model_count / model_graph: every round is all_contigs on the current
solid set, then the rule below on (G, contig lengths, dict counts, contig indices) alone.

  len_i, W_i, S_i  len(r[i]); len_i - k + 1; the sum of d[r[i][p:p+k]] over its W_i windows (dict
                   counts: a palindromic k-mer's count already holds 2 per occurrence)
  port             a link (j, o) reaches the port (j, t), t = 1 if o == '+' else 0
  branch i         len_i <= max_bubble_len (0: 2 k), |G[i][0]| == 1 and |G[i][1]| == 1, its two
                   ports P0, P1 differ and neither port's contig is i itself
  partner i2 != i  a branch whose unordered pair of ports equals {P0, P1} (either orientation)
  popped           some partner i2 has S_i2 W_i > S_i W_i2 (a strictly higher mean coverage,
                   compared exactly in integers), or equality there and i2 < i
  popping          removes every k-mer window of r[i], and its twin, from the dict; the first
                   events (the order) of the remaining entries stay
"""
from model_parallel import model_count, model_graph, twin


def ksums(contigs, d, k):
    """S_i per contig; d: the dict as [[k-mer, count], ...] or a mapping"""
    dd = dict((x, c) for x, c in d) if not hasattr(d, "get") else d
    return [sum(dd[c[p:p + k]] for p in range(len(c) - k + 1)) for c in contigs]


def ports_of(contigs, links, k, max_bubble_len=0):
    """per contig the sorted pair of its ports (port (j, t) as 2 j + t), or None if no branch"""
    mb = max_bubble_len or 2 * k
    out = []
    for i, c in enumerate(contigs):
        key = None
        if len(c) <= mb and len(links[i][0]) == 1 and len(links[i][1]) == 1:
            (j0, o0), (j1, o1) = links[i][0][0], links[i][1][0]
            p0, p1 = 2 * j0 + (1 if o0 == "+" else 0), 2 * j1 + (1 if o1 == "+" else 0)
            if p0 != p1 and j0 != i and j1 != i:
                key = (min(p0, p1), max(p0, p1))
        out.append(key)
    return out


def popped_of(contigs, links, d, k, max_bubble_len=0, sums=None):
    """indices of the contigs the rule pops in (links, contigs) = all_contigs' (G, r) of dict d;
    sums: S_i given directly (hand-written cases) instead of computed from d"""
    S = list(sums) if sums is not None else ksums(contigs, d, k)
    W = [len(c) - k + 1 for c in contigs]
    key = ports_of(contigs, links, k, max_bubble_len)
    groups = {}
    for i, q in enumerate(key):
        if q is not None:
            groups.setdefault(q, []).append(i)
    out = []
    for i, q in enumerate(key):
        if q is None:
            continue
        for i2 in groups[q]:
            if i2 == i:
                continue
            a, b = S[i2] * W[i], S[i] * W[i2]
            if a > b or (a == b and i2 < i):
                out.append(i)
                break
    return out


def pop_solid(cnt, first, k, max_bubble_len=0, max_rounds=4):
    """The loop on a solid set (cnt: canonical -> count, first: string -> first event).
    Returns (dict items, contigs, links, info, history): info as ec_pop_info, history one
    (contigs before the round, contigs popped, k-mers removed) per popping round."""
    solid = dict(cnt)
    d, contigs, links = model_graph(solid, first, k)
    info = {"rounds": 0, "converged": 0, "n_bubble_contigs": 0, "n_bubble_kmers": 0}
    history = []
    for _ in range(max_rounds):
        pop = popped_of(contigs, links, d, k, max_bubble_len)
        if not pop:
            info["converged"] = 1
            break
        nk = 0
        for i in pop:
            c = contigs[i]
            for p in range(len(c) - k + 1):
                x = c[p:p + k]
                solid.pop(min(x, twin(x)), None)
                nk += 1
        history.append((len(contigs), len(pop), nk))
        info["rounds"] += 1
        info["n_bubble_contigs"] += len(pop)
        info["n_bubble_kmers"] += nk
        d, contigs, links = model_graph(solid, first, k)
    return d, contigs, links, info, history


def pop_reads(reads, k, limit=1, max_bubble_len=0, max_rounds=4):
    cnt, first = model_count(reads, k)
    solid = {c: v for c, v in cnt.items() if v > limit}
    return pop_solid(solid, first, k, max_bubble_len, max_rounds)


def pop_dict(d, k, max_bubble_len=0, max_rounds=4):
    """The loop on a caller's ordered dict {k-mer: count} (closed under twin, as build returns
    it): entry i's first event is i."""
    first = {x: i for i, x in enumerate(d)}
    cnt = {min(x, twin(x)): v for x, v in d.items()}
    return pop_solid(cnt, first, k, max_bubble_len, max_rounds)


# ---- the hand-built case -----------------------------------------------------------------------
def _step(c, n=1):
    return "ACGT"[("ACGT".index(c) + n) % 4]


def hand_reads(k):
    """A 400-base genome read 4 times, a SNP at base 200 read 3 times, and a branch read twice
    that differs at 200 - s, 200 and 200 + s (s = k - 5): a SNP bubble nested inside a longer
    one.  For k = 33 the long branch has 89 windows, more than a wave."""
    from synth import make_genome

    g = make_genome(400, 7).decode()
    s = k - 5
    B = g[:200] + _step(g[200]) + g[201:]
    D = list(g)
    D[200 - s] = _step(g[200 - s])
    D[200] = _step(g[200], 2)
    D[200 + s] = _step(g[200 + s])
    D = "".join(D)
    return [g] * 4 + [B[200 - 2 * k:200 + 2 * k]] * 3 + [D[200 - s - 2 * k:200 + s + 2 * k]] * 2


def two_haplotype_reads(L, seed, glen=3000, na=1300, nb=520):
    """Error-free reads of length L from a glen-base genome (na) and from a second haplotype (nb)
    that carries a SNP every 260 bases from 150 on and one 1-base deletion: uniform starts, half
    reverse-complemented, shuffled."""
    import numpy as np
    from synth import make_genome

    A = make_genome(glen, seed).decode()
    Bl = list(A)
    for p in range(150, glen, 260):
        Bl[p] = _step(A[p])
    del Bl[glen // 2 + 17]
    B = "".join(Bl)
    rng = np.random.Generator(np.random.PCG64(seed))
    reads = []
    for hap, n in ((A, na), (B, nb)):
        for st in rng.integers(0, len(hap) - L + 1, n):
            reads.append(hap[int(st):int(st) + L])
    flip = rng.random(len(reads)) < 0.5
    reads = [twin(r) if f else r for r, f in zip(reads, flip)]
    return [reads[i] for i in rng.permutation(len(reads))]
