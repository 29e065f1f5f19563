"""bench.py's command line: a plain run does the headline only, --steps sets the timed steps,
--dump-outputs writes the last timed step's results (checked against the oracle on the same
reads).  One tiny-config run, shared by the tests."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from synth import make_reads

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("bench")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--config", "tiny",
                        "--dump-outputs", str(d / "dump")], cwd=str(d), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, "stdout carries exactly one JSON line"
    return json.loads(lines[0]), d / "dump"


def test_plain_result_line(plain_run):
    out, _ = plain_run
    assert out["steps"] == 3 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["unit"] == "k-mers/s" and out["higher_is_better"] is True and out["dtype"] == "u64"
    assert out["ms_per_step"] > 0
    # value = the job's k-mer positions / one step's wall time (both rounded in the line)
    assert out["value"] == pytest.approx(out["config"]["positions"] / (out["ms_per_step"] / 1e3), rel=1e-2)
    # the legs with runs of their own are --full's
    assert out["full"] is False
    for key in ("stage_ms", "cpu_baseline", "host_input", "host_input_value", "strong"):
        assert out[key] is None, key
    assert out["roofline"]["kernel_ms"] > 0  # (from the timed steps' kernel events)


def test_dumped_outputs_match_oracle(plain_run):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench

    _, dump = plain_run
    cfg = bench.CONFIGS["tiny"]
    buf, off = make_reads(cfg["genome"], cfg["reads"], cfg["read_len"], cfg["seed"])
    ref = oracle.assemble_packed(buf, off, cfg["k"], 1)
    got = {f[:-4]: np.load(str(dump / f)) for f in sorted(os.listdir(str(dump)))}
    # an empty array gets no file: link_codes is there only if the graph has links
    names = ["contig_chars", "contig_offsets"] + (["link_codes"] if len(ref["links"]) else []) + ["link_offsets"]
    assert sorted(got) == names and all(a.size for a in got.values())
    assert got["contig_chars"].dtype == np.float32
    assert all(got[n].dtype == np.float64 for n in names[1:])
    assert got["contig_chars"].astype(np.uint8).tobytes() == ref["contig_chars"]
    assert np.array_equal(got["contig_offsets"], ref["contig_offsets"].astype(np.float64))
    assert np.array_equal(got["link_offsets"], ref["link_offsets"].astype(np.float64))
    if len(ref["links"]):
        assert np.array_equal(got["link_codes"], ref["links"].astype(np.float64))
