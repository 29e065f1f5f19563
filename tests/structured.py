"""Seeded read sets over structured genomes: many circular replicons, repeat families, a
diploid pair, tandem repeats with hairpins, and k-mers seen more than 65 535 times.

synth.make_reads draws one iid-uniform genome, whose de Bruijn graph is near-linear; these
families put real topology (cycles, repeat junctions, solid bubbles, inverted repeats, heavy
keys) on inputs large enough to cross the ranking tiles, count buckets and rank segments.

Every function returns (buf uint8, offsets uint64) of ASCII reads of one length without N, as
make_reads does.  Reads are sampled with coverage proportional to the replicon's length, half
of them reverse-complemented; circular replicons wrap (a read longer than the replicon goes
round it more than once).  numpy PCG64, seeded; no files read."""
import numpy as np

from synth import LUT, make_reads

# circular replicon sizes around the ranking strides: RT_STEP_SEG = 512, RT_STEP = 768,
# RT_TN / 2 = 1024 canonical ids (RT_TN = 2048 oriented nodes), and half / 1.5x / 2x of them
REPLICON_SIZES = (383, 384, 385, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025, 1500, 2047, 2048, 2049,
                  3000, 5000)
HEAVY_UNITS = ("A", "AT", "CG", "AAC", "ACGT")


def _rng(*seed):
    return np.random.Generator(np.random.PCG64([int(s) for s in seed]))


def _rand(rng, n):
    return rng.integers(0, 4, int(n), dtype=np.uint8)


def _rc(x):
    return (3 - x[::-1]).astype(np.uint8)


def _codes(s):
    return np.array(["ACGT".index(c) for c in s], dtype=np.uint8)


def _pack(rows):
    n, L = rows.shape
    return LUT[rows].reshape(-1), np.arange(n + 1, dtype=np.uint64) * np.uint64(L)


def sample_reads(replicons, L, cov, rng):
    """replicons: list of (codes uint8[n], circular).  round(cov * n / L) reads (at least one) of
    every replicon, starts uniform (anywhere on a circular replicon, where the read fits on a
    linear one), half reverse-complemented, the reads of all replicons shuffled together."""
    ext, base, span, cnt = [], [], [], []
    at = 0
    for g, circ in replicons:
        n = len(g)
        assert circ or n >= L
        e = np.resize(g, n + L - 1) if circ else g  # (np.resize repeats g: the wrap)
        ext.append(e)
        base.append(at)
        span.append(n if circ else n - L + 1)
        cnt.append(max(1, int(round(cov * n / L))))
        at += len(e)
    G = np.concatenate(ext)
    rep = np.repeat(np.arange(len(replicons)), cnt)
    rng.shuffle(rep)
    starts = np.asarray(base)[rep] + (rng.random(len(rep)) * np.asarray(span)[rep]).astype(np.int64)
    rows = G[starts[:, None] + np.arange(L)[None, :]]
    flip = rng.random(len(rep)) < 0.5
    rows[flip] = 3 - rows[flip][:, ::-1]
    return _pack(rows)


def replicon_sizes(k, seed):
    """(sizes of the circular replicons, sizes of the linear ones) of replicons(k, seed)"""
    rng = _rng(seed, 1)
    circ = [n for n in REPLICON_SIZES if n >= k + 2] + [int(n) for n in rng.integers(k + 2, 1500, 150)]
    return circ, [700, 4000]


def replicons(k, seed):
    """~140 kbp in 168 circular replicons (plasmid-like: every one a cycle and its twin in the
    graph, sizes on and around the ranking strides and down to k + 2) and two linear ones;
    150 bp reads at 60x."""
    circ, lin = replicon_sizes(k, seed)
    rng = _rng(seed, 2)
    reps = [(_rand(rng, n), True) for n in circ] + [(_rand(rng, n), False) for n in lin]
    return sample_reads(reps, 150, 60, rng)


def repeat_families(k, seed):
    """~90 kbp genome with interspersed copies of seven repeat families, of lengths k - 1 (no
    shared k-mer, a shared (k-1)-mer junction only), k, k + 1, 2k, 300, 1200 and 12, in 30, 30, 30,
    40, 40, 10 and 50 copies; a copy is reverse-complemented with p = 0.4 and carries 1..3
    substitutions with p = 0.5.  Random spacers; 120 bp reads at 40x."""
    rng = _rng(seed, 3)
    lens = (k - 1, k, k + 1, 2 * k, 300, 1200, 12)
    copies = (30, 30, 30, 40, 40, 10, 50)
    fam = [_rand(rng, n) for n in lens]
    order = np.repeat(np.arange(len(lens)), copies)
    rng.shuffle(order)
    parts = [_rand(rng, rng.integers(100, 420))]
    for f in order:
        c = fam[f].copy()
        if rng.random() < 0.5:
            pos = rng.integers(0, len(c), int(rng.integers(1, 4)))
            c[pos] = (c[pos] + rng.integers(1, 4, len(pos), dtype=np.uint8)) & 3
        if rng.random() < 0.4:
            c = _rc(c)
        parts.append(c)
        parts.append(_rand(rng, rng.integers(100, 420)))
    return sample_reads([(np.concatenate(parts), False)], 120, 40, rng)


def diploid(k, seed):
    """two 40 kbp haplotypes that differ by substitutions at rate 1/60, covered equally: every
    bubble is solid on both arms (an error bubble has one thin arm).  120 bp reads at 40x each."""
    rng = _rng(seed, 4)
    a = _rand(rng, 40_000)
    b = a.copy()
    m = rng.random(len(a)) < 1.0 / 60
    b[m] = (b[m] + rng.integers(1, 4, int(m.sum()), dtype=np.uint8)) & 3
    return sample_reads([(a, False), (b, False)], 120, 40, rng)


def tandem_hairpin(k, seed):
    """60 blocks of spacer, unit^(2..5), spacer, arm, gap(0..7), rc(arm): tandem repeats with
    units of [k/2, 4k) bases (shorter than k: a cycle inside the read path) and inverted repeats
    with arms of [k, 5k) bases (the path turns back into its own twin).  ~80 kbp; 120 bp reads
    at 40x."""
    rng = _rng(seed, 5)
    parts = []
    for _ in range(60):
        unit = _rand(rng, rng.integers(k // 2, 4 * k))
        arm = _rand(rng, rng.integers(k, 5 * k))
        parts += [_rand(rng, rng.integers(300, 600)), np.tile(unit, int(rng.integers(2, 6))),
                  _rand(rng, rng.integers(300, 600)), arm, _rand(rng, rng.integers(0, 8)), _rc(arm)]
    return sample_reads([(np.concatenate(parts), False)], 120, 40, rng)


def _unit_read(unit, phase, L):
    u = _codes(unit)
    return np.resize(np.roll(u, -phase), L)


def heavy(k, L=None, seed=1, aligned=False):
    """make_reads(20_000, 4_000, L, seed) plus identical reads over the units A, AT, CG, AAC and
    ACGT, whose few canonical k-mers are then seen more than 65 535 times (a 16-bit bin wraps).
    aligned False (L = 100): 1 500 reads per unit, spread over the unit's phases, shuffled into
      the background: (L - k + 1) * 1500 windows per unit, over many read groups.
    aligned True (L = k + 289): every unit is one block of 256 identical reads that starts at a
      read index that is a multiple of 256, so one 256-read tile holds 256 * 290 = 74 240 windows
      of one canonical key; the block of unit A is half poly-A, half poly-T reads (one canonical
      key).  heavy_blocks() gives the blocks' first reads."""
    if L is None:
        L = k + 289 if aligned else 100
    bbuf, _ = make_reads(20_000, 4_000, L, seed)
    bg = bbuf.reshape(4_000, L)
    rng = _rng(seed, 6)
    if not aligned:
        rows = [bg]
        for u in HEAVY_UNITS:
            for p in range(len(u)):
                rows.append(np.tile(LUT[_unit_read(u, p, L)], (1500 // len(u), 1)))
        rows = np.concatenate(rows)
        rng.shuffle(rows)
        return rows.reshape(-1).copy(), np.arange(len(rows) + 1, dtype=np.uint64) * np.uint64(L)
    out = np.empty((4_000 + 256 * len(HEAVY_UNITS), L), np.uint8)
    first = heavy_blocks()
    free = np.ones(len(out), bool)
    for u, a in zip(HEAVY_UNITS, first):
        out[a:a + 256] = LUT[_unit_read(u, 0, L)]
        if u == "A":
            out[a + 128:a + 256] = LUT[_rc(_unit_read(u, 0, L))]
        free[a:a + 256] = False
    out[free] = bg
    return out.reshape(-1), np.arange(len(out) + 1, dtype=np.uint64) * np.uint64(L)


def heavy_blocks():
    """first read of every unit's block in heavy(aligned=True), in HEAVY_UNITS order"""
    return [256 * (1 + 3 * i) for i in range(len(HEAVY_UNITS))]


FAMILIES = {"replicons": replicons, "repeat_families": repeat_families, "diploid": diploid,
            "tandem_hairpin": tandem_hairpin}


# ---- the committed inputs and their reference results, shared by the test modules ---------------
SEED = 1
_INPUT = {}
_REF = {}


def reads_of(family, k):
    """(buf, offsets) of a family at k and the committed seed; family "heavy" / "heavy_aligned"
    for the two heavy sets.  Built once per module run, never modified."""
    key = (family, k)
    if key not in _INPUT:
        if family == "heavy":
            buf, off = heavy(k, 100, SEED, False)
        elif family == "heavy_aligned":
            buf, off = heavy(k, k + 289, SEED, True)
        else:
            buf, off = FAMILIES[family](k, SEED)
        buf.setflags(write=False)
        off.setflags(write=False)
        _INPUT[key] = (buf, off)
    return _INPUT[key]


def reference(buf, off, k, limit):
    """oracle.assemble_packed with the dict, plus the forms the parity tests compare against:
    links_unpacked, and the dict as one byte string of k-mers in order (d_kmers) and a uint32
    array of counts (d_counts) -- the layout ec_copy_dict writes, compared without a Python loop
    over 3 * 10^5 items per case"""
    import oracle

    ref = oracle.assemble_packed(buf, off, k, limit, True)
    ref["links_unpacked"] = oracle.unpack_links(ref)
    ref["d_kmers"] = "".join(x for x, _ in ref["d"]).encode()
    ref["d_counts"] = np.array([c for _, c in ref["d"]], dtype=np.uint32)
    return ref


def oracle_of(family, k):
    """the 2-bit oracle's result (with the dict) on reads_of(family, k), cached"""
    key = (family, k)
    if key not in _REF:
        buf, off = reads_of(family, k)
        _REF[key] = reference(buf, off, k, 1)
    return _REF[key]
