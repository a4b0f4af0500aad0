"""bench.py's plain run and --dump-outputs.

CPU: the record -> float64 conversion is exact and the sample of reads is fixed, sorted and
within the size limit.  GPU: a plain run prints only the headline line, --steps sets the number
of timed steps, and the dumped records are the oracle's records of the same seeded reads."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.common import ROOT

import bench  # noqa: E402  (the repository root is on sys.path: tests/conftest.py)
from subread_amd.abi import MAPPING_DTYPE, SUBJUNC_DTYPE, BIG_MARGIN_WORDS

LIMIT = 64 * 1000 * 1000      # bytes of dump files in all
FULL_ONLY = ("roofline", "device_path", "ascii_host_path", "sublong_voting", "cpu_baseline", "parity_check")


def test_records_as_float_is_exact():
    a = np.zeros((4, 2, 3), MAPPING_DTYPE)
    a["selected_position"] = 0xFFFFFFFF
    a["result_flags"] = -32768
    a["indels_in_confident_coverage"] = -128
    a["noninformative_subreads_in_vote"] = 255
    a["selected_indel_record"] = np.arange(22, dtype=np.int16) - 11
    a["confident_coverage_end"] = 65535
    a["_pad1"] = 0xABCD
    f = bench.records_as_float(a)
    assert f.dtype == np.float64 and f.shape == (4, 2, 3, 35)
    assert (f[..., 0] == 4294967295.0).all() and (f[..., 1] == -32768).all()
    assert (f[..., 5] == 255).all() and (f[..., 6] == -128).all()
    assert (f[..., 9:31] == np.arange(22) - 11).all()
    assert (f[..., 32] == 65535).all() and (f[..., 34] == 0xABCD).all()
    assert bench.records_as_float(np.zeros((2, 1, 3), SUBJUNC_DTYPE)).shape == (2, 1, 3, 9)
    w = np.arange(18, dtype=np.uint16).reshape(2, 1, 9)
    assert (bench.records_as_float(w) == w).all()


def test_dump_sample_is_fixed_sorted_and_fits():
    # the largest row of any workload: subjunc PE (2 ends x 3 bests of mapping + subjunc, big margin)
    row = 8 * (1 + 2 * 3 * 35 + 2 * 3 * 9 + 2 * BIG_MARGIN_WORDS)
    for n, rb in ((50_000_000, 8 * (1 + 3 * 35)), (25_000_000, row)):
        i = bench.dump_sample(n, rb)
        assert (i == bench.dump_sample(n, rb)).all()
        assert i.dtype == np.int64 and (np.diff(i) > 0).all() and i[0] >= 0 and i[-1] < n
        assert len(i) * rb <= LIMIT and len(i) >= 10000
    assert (bench.dump_sample(1000, row) == np.arange(1000)).all()


def test_dump_outputs_files(tmp_path):
    rng = np.random.default_rng(1)
    n = 3000
    out = np.frombuffer(rng.bytes(n * 3 * 68), dtype=MAPPING_DTYPE).reshape(n, 1, 3)
    assert bench.dump_outputs(str(tmp_path / "d"), {"mapping": out, "subjunc": None, "big_margin": None}) == n
    assert sorted(os.listdir(tmp_path / "d")) == ["mapping.npy", "sample_index.npy"]
    m = np.load(tmp_path / "d" / "mapping.npy")
    assert m.dtype == np.float64 and (m == bench.records_as_float(out)).all()
    assert (np.load(tmp_path / "d" / "sample_index.npy") == np.arange(n)).all()
    assert (m[..., 0] == out["selected_position"]).all()


def test_kernel_record_needs_full():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--kernel-record", "x.json"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--full" in r.stderr


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_plain_run_line_and_dump_match_oracle(tmp_path):
    n = 20000
    env = dict(os.environ, SVG_BENCH_DIR=str(tmp_path / "wd"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--workload", "c2", "--reads", str(n), "--dump-outputs", str(tmp_path / "dump")],
                       capture_output=True, text=True, env=env, timeout=110, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert not [k for k in FULL_ONLY if k in line]
    assert line["steps"] == 3 and len(line["host_step_ms"]) == 3 and line["warmup"] == 1
    assert line["unit"] == "Mreads/s" and line["higher_is_better"] is True and line["dtype"] == "u32"
    assert line["ms_per_step"] > 0
    # value is reads per timed step over ms_per_step; both are rounded to 3 decimals in the line
    tol = line["value"] * 0.0005 / line["ms_per_step"] + 0.0005
    assert abs(line["value"] - n / line["ms_per_step"] / 1e3) <= 1.01 * tol
    assert sorted(os.listdir(tmp_path / "dump")) == ["mapping.npy", "sample_index.npy"]
    got = np.load(tmp_path / "dump" / "mapping.npy")
    assert (np.load(tmp_path / "dump" / "sample_index.npy") == np.arange(n)).all()
    # the same seeded reads (bench.py workload c2) through the oracle, on the index files the run built
    from oracle.pyoracle import OracleIndex
    from subread_amd.abi import default_params, PROGRAM_ALIGN
    from subread_amd.sim import random_genome, simulate_reads
    rb = simulate_reads(random_genome([1_000_000], 901), n, 100, seed=20261015, first=0, sub=0.01, indel=0.001)
    ref = OracleIndex(str(tmp_path / "wd" / "genome_full")).vote(default_params(PROGRAM_ALIGN, False), rb, threads=4)[0]
    assert got.dtype == np.float64 and got.shape == (n, 1, ref.shape[2], 35)
    assert (got == bench.records_as_float(ref)).all()
