"""CPU statement (test infrastructure, pure Python, small cases only) of the coverage-aware solid
threshold that ec_kmer_spectrum / ec_spectrum_threshold / ec_refilter implement.

  spectrum   h[c] = canonical k-mers of the dict with dict count c (a palindrome's count already
             holds 2 per occurrence), h[nbins - 1] those with nbins - 1 or more
  threshold  on h[0 .. nbins-1], integers only:
               lo           the smallest c with h[c] > 0; none: not found
               descent_end  d = the smallest c in [lo, nbins-2] with h[c] < h[c+1]; not found if
                            there is none or d == lo
               peak         p = argmax of h[c] over [d, nbins-1], the smallest c on ties; not found
                            if p == nbins-1
               floor        m = min h[lo .. p]
               limit        v = the smallest c in [lo, p] with 16 (h[c] - m) <= h[p] - m; not found
                            if v == p
             not found: found = 0, limit = 0, the other fields as far as computed, 0 otherwise
  refilter   the ordered dict filtered by count > L (what build(limit=L) is: a filter on an
             insertion-ordered dict), then all_contigs on it (model_parallel.model_graph)
"""
from model_parallel import model_graph, twin

FLOOR_DIV = 16

# the fixed read sets of test_spectrum.py: synth.make_reads(G, n, L, seed, err=e), limit 1, 256 bins
# (G, n, L, seed, err, k) -> (found, lo, d, p, floor, limit, n_solid, kept)
FIXED = [
    ((3000, 1800, 100, 5, 0.01, 21), (1, 2, 4, 36, 0, 4, 4565, 2967)),
    ((3000, 1200, 100, 6, 0.005, 23), (1, 2, 3, 28, 1, 3, 3291, 2954)),
    ((2000, 600, 80, 7, 0.01, 15), (1, 2, 4, 16, 5, 3, 2106, 1931)),
    ((3000, 2400, 100, 8, 0.02, 31), (1, 2, 7, 32, 2, 5, 8236, 2943)),
    ((3000, 2400, 100, 8, 0.02, 33), (1, 2, 6, 29, 2, 5, 7922, 2940)),
    ((3000, 300, 100, 9, 0.01, 21), (0, 2, 2, 0, 0, 0, 2895, 2895)),
]


def info_of(found, lo, d, p, floor, limit):
    return {"found": found, "lo": lo, "descent_end": d, "peak": p, "limit": limit, "floor": floor}


def spectrum(d, nbins):
    """d: the ordered dict as [[k-mer, count], ...] or a mapping; every canonical k-mer once"""
    items = d.items() if hasattr(d, "items") else d
    h = [0] * nbins
    for x, c in items:
        if x <= twin(x):
            h[min(int(c), nbins - 1)] += 1
    return h


def threshold(h):
    h = [int(x) for x in h]
    n = len(h)
    info = {"found": 0, "lo": 0, "descent_end": 0, "peak": 0, "limit": 0, "floor": 0}
    lo = next((c for c in range(n) if h[c] > 0), None)
    if lo is None:
        return info
    info["lo"] = lo
    d = next((c for c in range(lo, n - 1) if h[c] < h[c + 1]), None)
    if d is None:
        return info
    info["descent_end"] = d
    if d == lo:
        return info
    p = max(range(d, n), key=lambda c: (h[c], -c))
    info["peak"] = p
    if p == n - 1:
        return info
    m = min(h[lo:p + 1])
    info["floor"] = m
    v = next(c for c in range(lo, p + 1) if FLOOR_DIV * (h[c] - m) <= h[p] - m)
    if v == p:
        return info
    info["found"] = 1
    info["limit"] = v
    return info


def filter_dict(d, L):
    """[[k-mer, count], ...] in order, the entries with count > L"""
    items = d.items() if hasattr(d, "items") else d
    return [[x, int(c)] for x, c in items if int(c) > L]


def refilter(d, k, L):
    """(dict items, contigs, links) of the dict filtered by count > L: entry i's first event is
    its position in d, as all_contigs reads a caller's dict"""
    items = [[x, int(c)] for x, c in (d.items() if hasattr(d, "items") else d)]
    first = {x: i for i, (x, _) in enumerate(items)}
    cnt = {min(x, twin(x)): c for x, c in items if c > L}
    return model_graph(cnt, first, k)
