"""A session's device memory is what it says it is (csrc/session.h: one list of buffers).

ec_mem_stats counts every byte a session buffer allocates and frees; ec_session_bytes sums the
buffers the session lists, ec_session_trim releases them and ec_session_destroy frees them.  On a
session of its own, after each path through the count and graph phases, the two agree exactly; a
trim(0) leaves at most the scalars block, and a closed session leaves nothing behind -- so a buffer
that is allocated but not listed (never counted, trimmed or freed) fails here."""
import pytest

import eulerhip
from synth import make_reads

pytestmark = pytest.mark.gpu

SHAPE = (20_000, 6_000, 100)  # genome, reads, read length (as smoke()); err = 0.002


@pytest.fixture(scope="module")
def reads():
    """(buf, off): plain reads, reads with N bytes, reads with one byte outside ACGTN"""
    plain = make_reads(*SHAPE, 5151, err=0.002)
    with_n = make_reads(*SHAPE, 5152, err=0.002, n_rate=0.001)
    ext = plain[0].copy()
    ext[37 * SHAPE[2] + 11] = ord("R")
    for b in (plain[0], with_n[0], ext):
        b.setflags(write=False)
    return {"plain": plain, "n": with_n, "ext": (ext, plain[1])}


def _run_host(s, r, k):
    s.run_host(*r, k, 1, 0)
    yield "run_host"


def _run_packed(s, r, k):
    s.run_packed_host(eulerhip.pack_2bit(*r), k, 1, 0)
    yield "run_packed_host"


def _clip_pop_spectrum(s, r, k):
    s.run_host(*r, k, 1, 0)
    yield "run_host"
    s.clip_tips(k)
    yield "clip_tips"
    s.pop_bubbles(k)
    yield "pop_bubbles"
    s.kmer_spectrum()
    yield "kmer_spectrum"


# name: (environment, reads, k, the calls -- a generator that yields after each of them)
CASES = {
    "default": ({}, "plain", 31, _run_host),
    "no_sk2": ({"EULERHIP_NO_SK2": "1"}, "plain", 31, _run_host),
    "rank_nodes": ({"EULERHIP_RANK": "1"}, "plain", 31, _run_host),
    "join_global": ({"EULERHIP_JOIN_LINKS": "1", "EULERHIP_JOIN_LOCAL": "0"}, "plain", 31, _run_host),
    "k51": ({}, "plain", 51, _run_host),
    "packed_host": ({}, "plain", 31, _run_packed),
    "n_bytes": ({}, "n", 31, _run_host),
    "extended": ({}, "ext", 31, _run_host),
    "clip_pop_spectrum": ({}, "plain", 31, _clip_pop_spectrum),
}


@pytest.mark.parametrize("case", list(CASES))
def test_held_bytes_are_the_listed_buffers(reads, monkeypatch, case):
    """after every call mem_stats' held bytes, less what was held before the session, equal
    device_bytes(); after trim(0) too, with at most the scalars block left"""
    env, which, k, calls = CASES[case]
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    held0 = eulerhip.mem_stats()[0]
    with eulerhip.Session(0) as s:
        for step in calls(s, reads[which], k):
            assert eulerhip.mem_stats()[0] - held0 == s.device_bytes(), step
        assert s.device_bytes() > 4096
        s.trim(0)
        assert eulerhip.mem_stats()[0] - held0 == s.device_bytes()
        assert s.device_bytes() <= 4096  # (all but the scalars)
    assert eulerhip.mem_stats()[0] == held0


def test_closed_session_holds_nothing(reads):
    """one stage_packed / assemble_staged round, then close(): the held bytes are back where they
    were before the session -- the staged slot's copies, outside device_bytes(), included"""
    held0 = eulerhip.mem_stats()[0]
    s = eulerhip.Session(0)
    try:
        pr = eulerhip.pack_2bit(*reads["plain"])
        s.stage_packed(pr)
        s.assemble_staged(31, 1, 0)
        assert s.stats().n_contigs > 0
    finally:
        s.close()
    assert eulerhip.mem_stats()[0] == held0
