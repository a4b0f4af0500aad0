"""CPU checks around svg_cell_parse_names and svg_cell_counter_tallies: the Python structures against the
header, the plain-C model (tests/native/cellname_model.c) on names outside the reference's contract
and on the tallies of crafted records (contig -1 first records among them), and the sanitizer program
(tests/native/cellname_check.c: the model against a restatement, no Python, no GPU)."""
import ctypes
import os
import re
import subprocess

import numpy as np

from subread_amd import abi
from tests.cellname_common import ASAN_CMD, BCL, CHECK_SRC, FASTQ, compose, model_parse, model_tallies
from tests.common import ROOT


def test_structs_match_header():
    src = open(os.path.join(ROOT, "include", "subread_vote.h")).read()
    for k, v in (("NAMES_BCL", abi.CELL_NAMES_BCL), ("NAMES_FASTQ", abi.CELL_NAMES_FASTQ), ("LANE_ALL", abi.CELL_LANE_ALL),
                 ("MAX_INDEX", abi.CELL_MAX_INDEX), ("NAME_STRIDE", abi.CELL_NAME_STRIDE), ("NAME_OK", abi.CELL_NAME_OK),
                 ("NAME_FEW_FIELDS", abi.CELL_NAME_FEW_FIELDS), ("NAME_PAST_END", abi.CELL_NAME_PAST_END), ("NAME_BAD_CHAR", abi.CELL_NAME_BAD_CHAR)):
        assert int(re.search(r"#define SVG_CELL_%s\s+(\d+)" % k, src).group(1)) == v
    body = re.search(r"typedef struct svg_cell_names \{(.*?)\} svg_cell_names;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for part in re.findall(r"\w+\s+([^;]+);", body) for n in re.findall(r"\*?(\w+)\s*(?:,|$)", part)]
    assert names == [f[0] for f in abi.SvgCellNames._fields_]
    assert ctypes.sizeof(abi.SvgCellNames) == 16 + 5 * 8 + 2 * ctypes.sizeof(abi.SvgPackedReads)
    assert [f[0] for f in abi.SvgCellSampleRow._fields_] == ["lane", "sample_no", "index"] and ctypes.sizeof(abi.SvgCellSampleRow) == 16


def test_model_outside_the_contract():
    for mode in (BCL, FASTQ):
        ok = compose(7, b"ACGTACGTACGTACGT" + b"AACCGGTTAACC", b"F" * 28, b"ACGTACGT", b"F" * 8, b"|@RgLater@L001", mode)
        names = [ok, ok[:13] + b"ACGT|FF", ok[:13 + 20] + b"!" + ok[13 + 21:], ok[:13] + b"ACGTACGTAC||", b"", b"R", ok[:40]]
        m = model_parse(names, mode, 16, 12)
        assert m["status"].tolist() == [0, 1, 3, 2, 1, 1, 1]
        assert (m["sample_no"][1:] == -1).all() and (m["lane"][1:] == -1).all() and (m["bc"][1:] == ord("A")).all()
        assert m["sample_no"][0] == 1 and m["lane"][0] == 1 and m["bc"][0].tobytes() == b"ACGTACGTACGTACGT"
        assert (m["packed"][1:] == 0).all() and m["packed"][0, 0] != 0


def test_model_tallies_on_crafted_records():
    """reads of 0, 1 and 3 records; a first record with contig -1 (an unmapped call although later
    records stand); nhits 0; samples 0 and -1"""
    heads = np.zeros(6, abi.CELL_ALN_HEAD_DTYPE)
    heads["n_records"] = [0, 1, 3, 3, 1, 2]
    heads["first_record"] = [0, 0, 1, 4, 7, 8]
    hits = np.zeros(10, abi.CELL_HIT_DTYPE)
    hits["contig"] = [0, 0, 1, 1, -1, 2, 2, 0, 0, -1]
    hits["nhits"] = [2, 0, 5, 5, 0, 3, 3, 1, 1, 0]
    t = model_tallies(heads, hits, [1, 1, 2, 2, 0, -1], None, 2)
    assert t.tolist() == [[2, 6, 3], [1, 1, 0], [1, 0, 0]]
    t = model_tallies(heads, hits, [1, 1, 2, 2, 0, 3], [0, 1, 0, 0, 0, 0], 2)      # a refused name, a sample above n_samples
    assert t.tolist() == [[1, 6, 1], [0, 1, 0], [0, 0, 0]]


def test_native_check_under_sanitizers(tmp_path):
    exe = str(tmp_path / "cellname_check")
    r = subprocess.run(ASAN_CMD + ["-o", exe, CHECK_SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "cellname_check OK" in r.stdout, r.stdout + r.stderr
