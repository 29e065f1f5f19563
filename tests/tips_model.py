"""CPU statement (test infrastructure, pure Python, small cases only) of the tip-clipping
contract that ec_clip_tips / Session.clip_tips / assembler.clip_tips implement on the device.

Built on model_parallel.model_count / model_graph: every round is all_contigs on the current
solid set, then the rule below on (G, contig lengths, contig indices) alone.

  candidate i   len(r[i]) <= max_tip_len (0: 2 k) and exactly one of G[i][0], G[i][1] is empty;
                a = its non-empty side
  siblings      per link (j, o) of G[i][a]: the entries (i2, _) of G[j][t], i2 != i, with
                t = 1 if o == '+' (j was entered at its head) else 0
  clipped       some sibling is no candidate, or longer, or as long with a smaller index
  clipping      removes every k-mer window of r[i], and its twin, from the dict; the first
                events (the order) of the remaining entries stay
"""
from model_parallel import model_count, model_graph, twin


def clipped_of(contigs, links, k, max_tip_len=0):
    """indices of the contigs the rule clips in (links, contigs) = all_contigs' (G, r)"""
    mt = max_tip_len or 2 * k
    n = len(contigs)
    ln = [len(c) for c in contigs]
    side = [None] * n  # the candidate's non-empty side
    for i in range(n):
        e0, e1 = not links[i][0], not links[i][1]
        if ln[i] <= mt and e0 != e1:
            side[i] = 1 if e0 else 0
    out = []
    for i in range(n):
        if side[i] is None:
            continue
        clip = False
        for j, o in links[i][side[i]]:
            for i2, _ in links[j][1 if o == "+" else 0]:
                if i2 == i:
                    continue
                if side[i2] is None or ln[i2] > ln[i] or (ln[i2] == ln[i] and i2 < i):
                    clip = True
        if clip:
            out.append(i)
    return out


def clip_solid(cnt, first, k, max_tip_len=0, max_rounds=4):
    """The loop on a solid set (cnt: canonical -> count, first: string -> first event).
    Returns (dict items, contigs, links, info, history): info as ec_clip_info, history one
    (contigs before the round, contigs clipped, k-mers removed) per clipping round."""
    solid = dict(cnt)
    d, contigs, links = model_graph(solid, first, k)
    info = {"rounds": 0, "converged": 0, "n_tip_contigs": 0, "n_tip_kmers": 0}
    history = []
    for _ in range(max_rounds):
        tips = clipped_of(contigs, links, k, max_tip_len)
        if not tips:
            info["converged"] = 1
            break
        nk = 0
        for i in tips:
            c = contigs[i]
            for p in range(len(c) - k + 1):
                x = c[p:p + k]
                solid.pop(min(x, twin(x)), None)
                nk += 1
        history.append((len(contigs), len(tips), nk))
        info["rounds"] += 1
        info["n_tip_contigs"] += len(tips)
        info["n_tip_kmers"] += nk
        d, contigs, links = model_graph(solid, first, k)
    return d, contigs, links, info, history


def clip_reads(reads, k, limit=1, max_tip_len=0, max_rounds=4):
    cnt, first = model_count(reads, k)
    solid = {c: v for c, v in cnt.items() if v > limit}
    return clip_solid(solid, first, k, max_tip_len, max_rounds)


def clip_dict(d, k, max_tip_len=0, max_rounds=4):
    """The loop on a caller's ordered dict {k-mer: count} (closed under twin, as build returns
    it): entry i's first event is i."""
    first = {x: i for i, x in enumerate(d)}
    cnt = {min(x, twin(x)): v for x, v in d.items()}
    return clip_solid(cnt, first, k, max_tip_len, max_rounds)


# ---- the hand-built case -----------------------------------------------------------------------
def _other(c):
    return "ACGT"[("ACGT".index(c) + 1) % 4]


def hand_reads(k, branch=12, seed=20261020):
    """A 400-base genome with a branch at base 200 that forks into a longer and a shorter tip,
    two equal-length tips at the genome's end and an isolated (k + 4)-mer, every read twice
    (limit 1).  branch: bases of the longer tip's own sequence X (12: the issue's case; 100 with
    max_tip_len 150: more than 64 windows a tip)."""
    from synth import make_genome

    g = make_genome(400, seed).decode()
    rnd = make_genome(branch + 2 + k + 4, seed + 1).decode()
    X = _other(g[200]) + rnd[:branch - 1]
    Y = _other(X[8]) + rnd[branch - 1:branch + 1]
    lone = rnd[branch + 1:branch + 1 + k + 4]
    reads = [g,
             g[200 - 2 * k:200] + X,
             g[200 - 2 * k:200] + X[:8] + Y,
             g[-2 * k:] + "ACG",
             g[-2 * k:] + "CTT",
             lone]
    return reads + reads


def n50(contigs):
    ls = sorted((len(c) for c in contigs), reverse=True)
    half, run = sum(ls) / 2.0, 0
    for x in ls:
        run += x
        if run >= half:
            return x
    return 0
