"""The (k, read length) grid over the compiled count-kernel variants: its tables, its inputs and
the count path the dispatch gives every cell.  Shared by test_kernel_grid.py (no GPU: the tables
reach every instantiation, every cell's reference result is non-trivial) and
test_kernel_grid_gpu.py (every cell bit-exact against the oracle, on the predicted path).

The dispatch, restated (functions of csrc/count_phase.h unless another file is named; L = the one
length of the reads that have windows, n = reads, M = L - k + 1 windows a read):

  k <= 32   phase_count_v2 stages 64-read wave tiles in NPF = 4 / 7 / 10 KiB a wave
            (its npf_of); with a stage (L <= 159)
              21 <= k <= 32  k_skpart_w<NPF, k - 14, VAL> (skpart_kernel, launched by
                             sk2_partition): VAL = true without a prescan when the first read has
                             windows (phase_count_v2's fast path), VAL = false after the prescan
                             when it is shorter than k (phase_count_v2, `if (allow_sk2)`)
              otherwise      k_partition<NPF, k >= 17, R10> (phase_count_v2, EC_PARTITION), R10 as
                             EULERHIP_V2_R10 forces it where k >= 16 (phase_count_v2, `r10`)
            without one (L >= 160: phase_count_v2 returns at `!npf`) count_part.h's exact path
            (phase_count); and after k_partition where the input has too few distinct keys for
            its fixed capacities (phase_count_v2's overflow / skew returns: k <= 4 here, see
            window_record_capacity_holds)
  k >= 33   phase_count_w: k <= 52 and k <= L <= 160 k_wbv<k - 14> and minimizer runs
            (phase_count_wpart, `mb`), else hash buckets on the staged upsweep (count_wide.h
            k_upsweep_w) while a 256-read tile fits STAGE_W bytes, else the HBM table
            (phase_count_wpart's `lens[2]` return, phase_count_w's table loop)
"""
import numpy as np

from synth import make_reads

GENOME = 3_000
NREADS = 1_300  # 20 * 64 + 20 = 5 * 256 + 20: the last wave tile and the last 256-read tile are partial
ERR = 0.002

EC_PATH_PARTITIONED, EC_PATH_GENERAL = 0, 1  # include/eulerhip.h

# the dispatch's constants (test_kernel_grid.py reads them back from the sources)
SK_M = 15            # superkmer.h: minimizer length; block width W = k - SK_M + 1 = k - 14
SK_MIN_K = 21        # superkmer.h
WMB_MAX_K = 52       # count_wide.h
WMB_MAXL = 160       # count_wide.h
STAGE_W = 40_896     # count_wide.h: stage of the wide upsweep / downsweep (256-read tiles)
STAGE_BYTES = 28_672  # count_part.h: stage of the exact path's tiles (256 reads)
TILE_READS = 256     # count_part.h


def npf_of(L):
    """staged KiB per wave of a 64-read tile of reads of <= L bases, 0: none (phase_count_v2, npf_of;
    the 30: up to 15 bytes before the tile's first byte and after its last one, rounding the
    16-byte loads)"""
    need16 = (64 * L + 30 + 15) // 16
    return 4 if need16 <= 4 * 64 else 7 if need16 <= 7 * 64 else 10 if need16 <= 10 * 64 else 0


def _tile_bytes(n, L):
    """bytes the 16-byte loads of the largest 256-read tile cover, in a 16-byte aligned buffer
    (a tile starts at a multiple of 256 L bytes)"""
    return (min(n, TILE_READS) * L + 15) // 16 * 16


FEW_KEYS_K = 6  # 4^k / 2 canonical keys: at most 2 080, fewer than a 3 000-base genome has windows


def _mix64(x):
    """common.h mix64 on a uint64 array"""
    x = x ^ (x >> np.uint64(29))
    x = x * np.uint64(0xbf58476d1ce4e5b9)  # (wraps mod 2^64)
    return x ^ (x >> np.uint64(32))


def window_record_capacity_holds(buf, off, k):
    """The fixed capacities of phase_count_v2's window records, evaluated on an input of reads of
    one length: they are sized for keys that a hash spreads evenly (count_v2.h:4-8, :25), and an
    input with fewer distinct keys than that needs -- k = 1 has two canonical keys for 32 coarse
    buckets -- outgrows them, by design; the call is then redone on the exact path.
    Both in count_phase.h's phase_count_v2:
      `cap`, and its return at `hsc.overflow`:  a (coarse bucket, 64-read group) run holds 5/4 of
                    its even share + 128 records (k_partition sets `overflow` past it,
                    count_v2.h:351)
      `fcap`, and its return at `hsc.skew`:  a final bucket holds 5/4 of its even share + 1024
                    records (k_refine2 sets `skew`); with <= 2 080 keys the estimate plans the 32
                    coarse buckets as the final ones (its `bbits` loop)
    The bucket of a key is the top 5 bits of mix64(key) (count_v2.h:306-311)."""
    n = len(off) - 1
    L = int(off[1] - off[0])
    assert k <= FEW_KEYS_K and np.all(np.diff(off.astype(np.int64)) == L)
    M = L - k + 1
    b = np.asarray(buf).reshape(n, L)
    code = (((b >> 1) ^ (b >> 2)) & 3).astype(np.uint64)  # A C G T -> 0 1 2 3 (window.h code2)
    fwd = np.zeros((n, M), np.uint64)
    rc = np.zeros((n, M), np.uint64)
    for t in range(k):
        fwd |= code[:, t:t + M] << np.uint64(2 * (k - 1 - t))
        rc |= (np.uint64(3) - code[:, t:t + M]) << np.uint64(2 * t)
    with np.errstate(over="ignore"):
        bucket = (_mix64(np.minimum(fwd, rc)) >> np.uint64(59)).astype(np.int64)
    group = (np.arange(n) // 64)[:, None]  # groups of one 64-read tile up to 2048 x 64 reads (phase_count_v2, G / gsize)
    runs = np.bincount((group * 32 + bucket).reshape(-1), minlength=32 * ((n + 63) // 64))
    cap = (64 * M * 5 // 4 + 31) // 32 + 128
    fcap = n * M * 5 // 4 // 32 + 1024
    return bool(runs.max() <= cap and np.bincount(bucket.reshape(-1), minlength=32).max() <= fcap)


def expected_path(k, L, n, no_sk2=False, r10=-1, reads=None):
    """(count_path, count_variant, record_bytes) the dispatch gives n reads of one length L >= k
    (reads shorter than k beside them change nothing below: the prescan takes the lengths of the
    reads with windows, count_v2.h:81-87).  no_sk2: EULERHIP_NO_SK2; r10: EULERHIP_V2_R10;
    reads: the (buf, offsets) counted where they are not reads_of(k, L, n) (looked at for
    k <= FEW_KEYS_K only).  Every rule cites its function of csrc/count_phase.h (assemble.hip
    where named)."""
    assert 1 <= k <= 63 and L >= k and n >= 1
    if k <= 32:  # assemble.hip, assemble: phase_count for k <= 32
        v2 = npf_of(L) != 0  # phase_count_v2, `if (!npf)`: a wave stage holds the tile
        if v2 and k <= FEW_KEYS_K:  # too few distinct keys for the fixed capacities: see there
            v2 = window_record_capacity_holds(*(reads or reads_of(k, L, n)), k)
        if v2:
            # sk2_shape: super-k-mer records (M <= 256, a group's windows < 2^24 and 2 n M < 2^32
            # hold for every input of this size; the estimate of so few keys plans no filter, sk2_plan)
            if SK_MIN_K <= k <= 32 and not no_sk2:
                return EC_PATH_PARTITIONED, 3, 16  # phase_count_sk2, its stats at `done = true`
            # (k > FEW_KEYS_K: >= 8 192 canonical keys and ~3 000 distinct ones in the input, ~94 a
            # coarse bucket: no run or bucket comes near 5/4 of its even share, phase_count_v2's
            # `cap` and `fcap`)
            # phase_count_v2, `r10`: 10-byte records only where forced (P < 2^26), k >= 16, and the
            # remnant fits: 2 k - 5 <= 59 bits, and the meta of 64-read groups (6 + 1 + ibits <= 15
            # bits) fits its 16-bit array
            on = r10 == 1 and k >= 16
            return EC_PATH_PARTITIONED, 2 if on else 1, 10 if on else 12  # phase_count_v2's stats
        # declined: count_part.h's exact path (phase_count): partitioned (its `part`: M <= 32 767,
        # est / 8192 <= 2400); compact 12-byte records only if every tile was staged (its `compact`:
        # lens[2] == 0, count_part.h:168), else 16-byte ones
        return EC_PATH_PARTITIONED, 0, 12 if _tile_bytes(n, L) <= STAGE_BYTES else 16
    # phase_count_w, `mb`: minimizer buckets for k <= WMB_MAX_K; phase_count_wpart, `if (mb)`: the
    # length they take, and its minimizer runs
    if k <= WMB_MAX_K and L <= WMB_MAXL:
        return EC_PATH_PARTITIONED, 0, 16
    # phase_count_w, hash buckets: 24-byte window records (phase_count_wpart) if every 256-read tile
    # fits the staged upsweep (count_wide.h:187 sets lens[2] otherwise; phase_count_wpart returns
    # at `hsc.lens[2]`), else the HBM table (phase_count_w's table loop, finish_wide)
    if _tile_bytes(n, L) <= STAGE_W:
        return EC_PATH_PARTITIONED, 0, 24
    return EC_PATH_GENERAL, 0, 0


# ---- the tables ---------------------------------------------------------------------------------
A_KS = tuple(range(21, 33))
A_EDGES = (63, 64, 111, 112, 159)  # the wave stage exactly full (63, 111, 159) / the next size
A_CELLS = [(k, L) for k in A_KS for L in (k, k + 1) + A_EDGES if L >= k]
A_LONG = [(21, 160), (27, 160), (32, 160)]  # past the largest stage: the exact path

B_LS = (40, 63, 64, 90, 111, 112, 140, 159)  # one length inside each NPF class and the class edges
B_DEFAULT_KS = (1, 2, 7, 8, 15, 16, 17, 20)
B_NO_SK2_KS = (16, 17, 23, 29, 32)
# (k, L, no_sk2, r10): r10 forced off and on where the dispatch can take it (k >= 16), else left
B_CASES = [(k, L, False, r) for k in B_DEFAULT_KS for L in B_LS for r in ((0, 1) if k >= 16 else (-1,))] + \
          [(k, L, True, r) for k in B_NO_SK2_KS for L in B_LS for r in (0, 1)]

C_KS = tuple(range(33, 64))
C_CELLS = [(k, L) for k in C_KS for L in (k, k + 1, 100, 159, 160, 161)]

D_NS = (1, 63, 64, 65, 255, 257)
D_CELLS = [(23, 111), (17, 112), (48, 100)]  # one cell of A, B and C

E_OFFSETS = (1, 7, 8, 15)
E_CELLS = [(23, 63), (17, 111), (48, 160)]  # one cell of A, B and C, each with its stage exactly full

F_KS = tuple(range(1, 64))
F_L = 100
F_SWITCH_KS = (20, 21, 32, 33, 52, 53, 63)  # both sides of merge_sk / merge_wmb / the owner rule


def skpart_form(k, L):
    """(NPF, W) of the k_skpart_w a super-k-mer cell runs"""
    return npf_of(L), k - SK_M + 1


def partition_form(k, L, r10):
    """(NPF, HI, R10) of the k_partition a window-record cell runs"""
    return npf_of(L), k >= 17, r10 == 1 and k >= 16


# ---- inputs and reference results ---------------------------------------------------------------
def seed_of(k, L):
    return 7_000_000 + 1_000 * k + L


def short_lengths(k, n):
    """{read: length < k} of the short variant: the first read (the dispatch looks at it alone,
    count_phase.h phase_count_v2's fast path), reads on both sides of a wave tile's edge, one inside, the last"""
    return {0: k - 1, 1: 0, 63: 1, 64: k // 2, n // 2: k - 1, n - 1: k - 2}


_INPUT = {}
_REF = {}


def reads_of(k, L, n=NREADS, short=False):
    """(buf, offsets): n reads of L bases over a 3 000-base genome; short: the reads of
    short_lengths(k, n) cut to fewer than k bases.  Built once, never modified."""
    key = (k, L, n, short)
    if key not in _INPUT:
        buf, off = make_reads(GENOME, n, L, seed_of(k, L), err=ERR)
        if short:
            lens = np.full(n, L, dtype=np.int64)
            for r, ln in short_lengths(k, n).items():
                lens[r] = ln
            buf = buf.reshape(n, L)[np.arange(L)[None, :] < lens[:, None]].copy()
            off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        buf.setflags(write=False)
        off.setflags(write=False)
        _INPUT[key] = (buf, off)
    return _INPUT[key]


TWO_LENGTH_KS = (33, 52)  # both ends of k_wbv's range
TWO_LENGTHS = (100, 150)


def two_length_reads(k):
    """(buf, offsets): 600 reads of 100 and 150 bases, the first one (whose length the minimizer
    buckets take for all, count_phase.h phase_count_wpart, `if (mb)`) among the shorter: every third read is cut"""
    key = ("two", k)
    if key not in _INPUT:
        n, (la, lb) = 600, TWO_LENGTHS
        buf, _ = make_reads(GENOME, n, lb, seed_of(k, 0), err=ERR)
        lens = np.where(np.arange(n) % 3 == 0, la, lb)
        buf = buf.reshape(n, lb)[np.arange(lb)[None, :] < lens[:, None]].copy()
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        buf.setflags(write=False)
        off.setflags(write=False)
        _INPUT[key] = (buf, off)
    return _INPUT[key]


def oracle_of_two_lengths(k):
    from structured import reference

    if ("two", k) not in _REF:
        _REF[("two", k)] = reference(*two_length_reads(k), k, 1)
    return _REF[("two", k)]


def oracle_of(k, L, n=NREADS, short=False, limit=1):
    """structured.reference (the 2-bit oracle with the dict) on reads_of(k, L, n, short), cached"""
    from structured import reference

    key = (k, L, n, short, limit)
    if key not in _REF:
        buf, off = reads_of(k, L, n, short)
        _REF[key] = reference(buf, off, k, limit)
    return _REF[key]
