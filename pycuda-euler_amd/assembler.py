"""assembler -- the reference CPU assembler's interface, GPU-backed.

Mirrors src/referenceassembler/referenceAssembler.py (and its twin tests/referenceAssembler.py):
the same names, arguments and results, with build() and all_contigs() running on the MI355X
through libeulerhip.so:

* build(reads, k, limit)  (:25-42)  -> the insertion-ordered dict {k-mer: count} of solid k-mers,
  produced by the fused counting path with the dict rendered on the device;
* all_contigs(d, k)       (:79-111) -> (G, r): contigs in the reference's order and the GFA link
  table, computed by the device graph phase from the caller's dict (any dict closed under
  twin, as build returns, in any order -- the order decides the contig order as in the
  reference);
* assemble(reads, k, limit) -> (d, G, r) in one fused device pass (no dict round trip);
* clip_tips(d, k) -> (d2, G, r): tip clipping on the device, which the reference does not have
  (also assemble(..., clip_tips=True); off by default);
* pop_bubbles(d, k) -> (d2, G, r): bubble popping on the device, likewise beyond the reference
  (also assemble(..., pop_bubbles=True); off by default; with both, tips are clipped first);
* assemble(..., auto_limit=True): beyond the reference, the solid limit read off the k-mer count
  spectrum of the assembly (eulerhip.spectrum_threshold) and applied on the device without a
  recount, before the tips and bubbles (off by default);
* kmer_spectrum(reads, k, limit) -> the count spectrum of build(reads, k, limit), beyond the
  reference;
* print_GFA / print_dbg (:115-130, with the working formatting of tests/referenceAssembler.py:119-134);
* twin / kmers / fw / bw / contig_to_string: the reference's string helpers (host, not on
  the hot path).

Documented deviation: k-mers with bytes other than A/C/G/T (after N-splitting) raise
eulerhip.AlphabetError (the reference keeps them as opaque strings; a 2-bit code cannot).
get_contig / get_contig_forward, the reference's serial per-k-mer walkers inside all_contigs,
are subsumed by the device graph phase and are not exposed.
"""
import argparse
import collections
import sys

import eulerhip

_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def twin(km):
    """:7-10 reverse complement (other characters map to themselves)."""
    return "".join(_COMP.get(c, c) for c in reversed(km))


def kmers(seq, k):
    """:12-14"""
    for i in range(len(seq) - k + 1):
        yield seq[i:i + k]


def fw(km):
    """:16-18"""
    for x in "ACGT":
        yield km[1:] + x


def bw(km):
    """:20-22"""
    for x in "ACGT":
        yield x + km[:-1]


def contig_to_string(c):
    """:44-45"""
    return c[0] + "".join(x[-1] for x in c[1:])


def _session(session):
    return session or eulerhip.default_session()


def build(reads, k=31, limit=1, session=None):
    """:25-42 -- the solid-k-mer dict in the reference's insertion order."""
    res = _session(session).assemble(list(reads), int(k), limit=limit, want_dict=True)
    return collections.OrderedDict(res.dict_items)


def all_contigs(d, k, session=None):
    """:79-111 -- (G, r) for the dict d."""
    res = _session(session).assemble_dict(d, int(k))
    return res.G(), res.contigs


def assemble(reads, k=31, limit=1, session=None, want_dict=True, clip_tips=False, pop_bubbles=False,
             auto_limit=False):
    """build + all_contigs in one device pass: (d, G, r).  auto_limit: the solid limit the k-mer
    count spectrum of the assembly suggests (eulerhip.spectrum_threshold) applied first, if one
    is found.  clip_tips / pop_bubbles: the tips clipped, then the bubbles popped, at the default
    settings (see clip_tips and pop_bubbles below).  All three go beyond the reference -- d is
    then the cleaned dict."""
    s = _session(session)
    res = s.assemble(list(reads), int(k), limit=limit, want_dict=want_dict)
    if auto_limit:
        res, _, _ = s.auto_limit(int(k), want_dict=want_dict)
    if clip_tips:
        res, _ = s.clip_tips(int(k), want_dict=want_dict)
    if pop_bubbles:
        res, _ = s.pop_bubbles(int(k), want_dict=want_dict)
    d = collections.OrderedDict(res.dict_items) if want_dict else None
    return d, res.G(), res.contigs


def kmer_spectrum(reads, k=31, limit=1, nbins=1024, session=None):
    """The k-mer count spectrum of build(reads, k, limit), which the reference does not report:
    np.uint64[nbins], hist[c] = canonical k-mers of the dict with count c, the last bin holding
    those with nbins - 1 or more (eulerhip.Session.kmer_spectrum)."""
    s = _session(session)
    s.assemble(list(reads), int(k), limit=limit)
    return s.kmer_spectrum(nbins)


def clip_tips(d, k, max_tip_len=None, max_rounds=4, session=None):
    """Graph clean-up the reference does not have: all_contigs(d, k), then the tips clipped on
    the device (eulerhip.Session.clip_tips; the rule is stated in include/eulerhip.h) -- short
    dead-end contigs of at most max_tip_len characters (None: 2 k) that have a longer, or equal
    and earlier, sibling at their junction, up to max_rounds rounds.  Returns (d2, G, r): the
    surviving dict in d's order and all_contigs(d2, k)."""
    s = _session(session)
    s.assemble_dict(d, int(k), keep_dict=True)
    res, _ = s.clip_tips(int(k), max_tip_len or 0, max_rounds, want_dict=True)
    return collections.OrderedDict(res.dict_items), res.G(), res.contigs


def pop_bubbles(d, k, max_bubble_len=None, max_rounds=4, session=None):
    """Graph clean-up the reference does not have: all_contigs(d, k), then the bubbles popped on
    the device (eulerhip.Session.pop_bubbles; the rule is stated in include/eulerhip.h) -- of
    parallel branches of at most max_bubble_len characters (None: 2 k) between the same two
    contig ends only the one with the highest mean count in d, or the earliest of equals, stays,
    up to max_rounds rounds.  Returns (d2, G, r): the surviving dict in d's order and
    all_contigs(d2, k)."""
    s = _session(session)
    s.assemble_dict(d, int(k), keep_dict=True)
    res, _ = s.pop_bubbles(int(k), max_bubble_len or 0, max_rounds, want_dict=True)
    return collections.OrderedDict(res.dict_items), res.G(), res.contigs


def print_GFA(G, cs, k, file=None):
    """:115-124 (tests/referenceAssembler.py:119-128 formatting)."""
    out = file or sys.stdout
    print("H  VN:Z:1.0", file=out)
    for i, x in enumerate(cs):
        print("S\t%d\t%s\t*" % (i, x), file=out)
    for i in G:
        for j, o in G[i][0]:
            print("L\t%d\t+\t%d\t%s\t%dM" % (i, j, o, k - 1), file=out)
        for j, o in G[i][1]:
            print("L\t%d\t-\t%d\t%s\t%dM" % (i, j, o, k - 1), file=out)


def print_dbg(cs, file=None):
    """:127-130 FASTA (tests/referenceAssembler.py:131-134 formatting)."""
    out = file or sys.stdout
    for i, x in enumerate(cs):
        print(">contig%d\n%s\n" % (i, x), file=out)


def read_fasta_records(path):
    """FASTA records with multi-line sequences joined (the SeqIO parsing of
    tests/referenceAssembler.py:28)."""
    seqs, cur = [], None
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line.startswith(">"):
                if cur is not None:
                    seqs.append("".join(cur))
                cur = []
            elif cur is not None:
                cur.append(line)
    if cur is not None:
        seqs.append("".join(cur))
    return seqs


def build_from_files(fns, k=31, limit=1, session=None):
    """tests/referenceAssembler.py:23-46 -- build over the records of FASTA files."""
    reads = []
    for fn in fns:
        reads.extend(read_fasta_records(fn))
    return build(reads, k, limit, session)


def runAssembler(k, src, session=None):
    """:135-140 -- build over a list of reads, print and return the dict."""
    d = build(src, k=int(k), session=session)
    print("done")
    print(d)
    return d


def main(argv=None):
    """A working CLI for src/assembler.py (whose own is non-functional):
    reads FASTA files, writes contigs as FASTA (print_dbg) or GFA (print_GFA)."""
    p = argparse.ArgumentParser(description="de Bruijn unitig assembler on MI355X")
    p.add_argument("inputs", nargs="+", help="FASTA files")
    p.add_argument("-k", type=int, default=31)
    p.add_argument("--limit", type=int, default=1, help="keep k-mers seen more than this many times")
    p.add_argument("--gfa", action="store_true", help="write GFA instead of FASTA")
    p.add_argument("-o", dest="output", default="", help="output file (default stdout)")
    a = p.parse_args(argv)
    reads = []
    for fn in a.inputs:
        reads.extend(read_fasta_records(fn))
    _, G, cs = assemble(reads, a.k, a.limit, want_dict=False)
    out = open(a.output, "w") if a.output else sys.stdout
    try:
        if a.gfa:
            print_GFA(G, cs, a.k, file=out)
        else:
            print_dbg(cs, file=out)
    finally:
        if a.output:
            out.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
