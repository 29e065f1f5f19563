"""bench.py's --dump-outputs writer on host arrays: dtypes, the byte budget, and the fixed sample
of an array past its share (no GPU)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


class _Result:
    def __init__(self, nchars):
        self.contig_bytes = np.random.default_rng(3).integers(65, 85, nchars, dtype=np.uint8).tobytes()
        self.contig_offsets = np.array([0, nchars // 3, nchars], np.uint64)
        self.link_offsets = np.array([0, 1, 2, 2, 3], np.uint64)
        self.link_codes = np.array([2, 3, (1 << 40) + 1], np.int64)


def _dump(tmp_path, name, res):
    d = str(tmp_path / name)
    bench.dump_outputs(d, res)
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}, sum(
        os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_whole_arrays(tmp_path):
    res = _Result(1001)
    got, _ = _dump(tmp_path, "a", res)
    assert got["contig_chars"].dtype == np.float32
    assert got["contig_chars"].astype(np.uint8).tobytes() == res.contig_bytes
    for n in ("contig_offsets", "link_offsets", "link_codes"):
        assert got[n].dtype == np.float64
        assert np.array_equal(got[n].astype(np.int64), np.asarray(getattr(res, n)).astype(np.int64)), n


def test_dump_skips_empty_arrays(tmp_path):
    res = _Result(1001)
    _dump(tmp_path, "a", res)
    res.link_offsets = np.zeros(5, np.uint64)
    res.link_codes = np.zeros(0, np.int64)
    got, _ = _dump(tmp_path, "a", res)  # the same directory: the earlier link_codes.npy goes
    assert sorted(got) == ["contig_chars", "contig_offsets", "link_offsets"]
    assert not got["link_offsets"].any()


def test_dump_samples_past_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET", 4096)
    res = _Result(10_007)  # 40 028 B as float32: past the budget; the three small arrays stay whole
    got, size = _dump(tmp_path, "a", res)
    again, _ = _dump(tmp_path, "b", res)
    assert sum(a.nbytes for a in got.values()) <= 4096 and size <= 4096 + 4 * 128
    assert np.array_equal(got["link_codes"], np.asarray(res.link_codes, np.float64))
    ch = got["contig_chars"]
    assert 900 < ch.size < 10_007 and all(np.array_equal(got[n], again[n]) for n in got)
    # the sample is one element of each of ch.size equal strata, in order
    chars = np.frombuffer(res.contig_bytes, np.uint8)
    stride = chars.size // ch.size
    assert all(v in chars[i * stride:(i + 1) * stride] for i, v in enumerate(ch.astype(np.uint8)))
