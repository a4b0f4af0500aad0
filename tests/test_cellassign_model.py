"""CPU checks of what svg_cell_assign_batch stands on: the record layouts against the header, the
host builder's refusals, the plain-C model's barcode rule against a scan of the whole whitelist,
the fixed cursor of cell-counts.c:2073-2083 against an advancing one, and the sanitizer program
(tests/native/cellassign_check.c: builder + model against full scans, no Python, no GPU).  The
model and the builder are pinned here to those scans and to a reading of the reference's code, not
to answers recorded from the reference."""
import ctypes
import os
import re
import subprocess

import numpy as np

from subread_amd import abi
from tests.cellassign_common import (ASAN_CMD, CHECK_SRC, brute_barcode, make_features, make_read_barcodes, make_whitelist,
                                     model_assign, model_barcodes, model_lib)
from tests.common import ROOT

PAD = 1210
CHR_END = np.cumsum([300000 + 2 * PAD - 16, 9000 + 2 * PAD - 16, 5000 + 2 * PAD - 16]).astype(np.uint32)


def test_structs_match_header():
    src = open(os.path.join(ROOT, "include", "subread_vote.h")).read()
    for name, dt, size in (("svg_cell_feature", abi.CELL_FEATURE_DTYPE, 20), ("svg_cell_hit", abi.CELL_HIT_DTYPE, 24)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for part in re.findall(r"\w+\s+([^;]+);", body) for n in re.findall(r"(\w+)(?:\[\w+\])?\s*(?:,|$)", part)]
        assert names == list(dt.names), name
        assert dt.itemsize == size
    assert [abi.CELL_HIT_DTYPE.fields[k][1] for k in abi.CELL_HIT_DTYPE.names] == [0, 4, 8, 12, 16]
    assert [abi.CELL_FEATURE_DTYPE.fields[k][1] for k in abi.CELL_FEATURE_DTYPE.names] == [0, 4, 8, 12, 16, 17]
    assert int(re.search(r"#define SVG_CELL_MAX_GENES\s+(\d+)", src).group(1)) == abi.CELL_MAX_GENES
    assert ctypes.sizeof(abi.SvgCellHits) == 32 and ctypes.sizeof(abi.SvgCellAssigned) == 32 + 32 + 8


def records(pos, cigars, flags=0):
    a = np.zeros(len(pos), abi.CELL_ALN_DTYPE)
    a["position"], a["cigar"], a["flags"] = pos, cigars, flags
    return a


def test_model_locates_and_clips():
    """the padding counts: a position inside a contig's leading padding, within 15 bases of the next
    contig's and beyond the last contig is unmapped; only a head S moves chro_pos"""
    e0 = int(CHR_END[0])
    a = records([PAD - 2, PAD - 1, PAD + 99, e0 + 15 - PAD - 1, e0 + 15 - PAD, e0 + PAD - 1, int(CHR_END[2]) + 5, PAD + 99, PAD + 99],
                [b"50M"] * 7 + [b"7S43M", b"43M7S"])
    hits, genes = model_assign(np.zeros(0, abi.CELL_FEATURE_DTYPE), 0, CHR_END, PAD, a)
    assert hits["contig"].tolist() == [-1, 0, 0, 0, -1, 1, -1, 0, 0]
    assert hits["chro_pos"].tolist() == [0, 0, 100, e0 + 15 - 2 * PAD, 0, 0, 0, 107, 100]
    assert len(genes) == 0 and (hits["nhits"] == 0).all()


def test_model_fixed_cursor_differs_from_an_advancing_one():
    f = np.array([(0, 1000, 1050, 7, 0, (0, 0, 0)), (0, 1100, 1150, 8, 0, (0, 0, 0)), (0, 1000, 1020, 7, 0, (0, 0, 0)),
                  (0, 1030, 1040, 9, 1, (0, 0, 0))], abi.CELL_FEATURE_DTYPE)
    a = records([PAD + 989] * 3, [b"30M80N40M", b"30M", b"200M"])   # chro_pos 990
    hits, genes = model_assign(f, 1, CHR_END, PAD, a)
    assert hits["nhits"].tolist() == [1, 1, 2] and genes.tolist() == [7, 7, 7, 8]
    adv, g2 = model_assign(f, 1, CHR_END, PAD, a, advance=True)
    assert adv["nhits"].tolist() == [2, 1, 2] and g2.tolist() == [7, 8, 7, 7, 8]
    none, g0 = model_assign(f, 0, CHR_END, PAD, a)          # the rule of :1982
    assert none["nhits"].tolist() == [1, 1, 0] and g0.tolist() == [7, 7]
    neg, g1 = model_assign(f, 1, CHR_END, PAD, records([PAD + 989], [b"60M"], 16))
    assert g1.tolist() == [9]


def test_model_barcodes_equal_a_scan_of_the_whitelist():
    rng = np.random.default_rng(1701)
    for L in (2, 5, 12, 16):
        wl = make_whitelist(min(300, 4 ** L // 2), L, rng)
        rd = make_read_barcodes(wl, 1200, rng)
        got = model_barcodes(wl, rd)
        want = np.array([brute_barcode(wl, r) for r in rd])
        assert (got == want).all(), L
        if L >= 12:
            for cls in range(6):
                assert (want[cls::6] >= 0).sum() >= 20 or cls == 3, (L, cls)
            assert (want[3::6] < 0).sum() >= 20


def test_barcode_f_row_wins_over_a_lower_s_row_entry():
    wl = [b"AAAACCCC", b"CATAAAAA", b"AAAAAAAT", b"AAAAAAAA"]
    #      read AAAAAAAC: S key AAAA -> entries 2, 3 at distance 1; F key AAAA -> entries 2, 3 as well
    assert model_barcodes(wl, [b"AAAAAAAC"]).tolist() == [2]
    wl = [b"ACAAAAAA", b"AAAAAAAG"]   # read AAAAAAAA: entry 0 has its F key (S row no), entry 1 its S key
    assert model_barcodes(wl, [b"AAAAAAAA", b"ANAAAAAA", b"NAAAAAAA", b"AAAAAANG"]).tolist() == [0, 0, -1, 1]
    # entry 0 differs at an even position (the read's S row), entry 1 at an odd one (its F row): the F row goes first
    assert model_barcodes([b"GAAAAAAA", b"AAAAAAAG"], [b"AAAAAAAA"]).tolist() == [1]


def test_builder_refusals():
    L = model_lib()
    hits = np.zeros(1, abi.CELL_HIT_DTYPE)
    g = np.zeros(64, np.int32)
    a = records([PAD + 10], [b"10M"])
    for bad in ((3, 10, 20, 0, 0), (0, 30, 20, 0, 0), (0, 10, 20, 0, 2), (2, 10, 5000 + 2 * PAD + 1400000, 0, 0)):
        f = np.array([bad + ((0, 0, 0),)], abi.CELL_FEATURE_DTYPE)
        k = L.cellassign_model_features(f.ctypes.data, 1, 0, 0, CHR_END.ctypes.data, 3, PAD, a.ctypes.data, 1, hits.ctypes.data, g.ctypes.data, 64)
        assert k == -2, bad
    out = np.zeros(1, np.int32)
    for wl, ln in (([b"ACGT", b"ACG"], 4), ([b"ACGN"], 4), ([b"A" * 17], 17), ([b"ACGT", b"ACGT"], 4), ([b"A"], 1)):
        buf = np.zeros((len(wl), ln + 1), np.uint8)
        for i, s in enumerate(wl):
            buf[i, :len(s)] = np.frombuffer(s, np.uint8)
        assert L.cellassign_model_barcodes(buf.ctypes.data, len(wl), ln, buf.ctypes.data, 0, out.ctypes.data) != 0, wl


def test_annotation_has_the_shapes_the_gpu_tests_need():
    f = make_features(CHR_END, PAD, np.random.default_rng(5))
    c0 = f[f["contig"] == 0]
    assert len(np.unique(c0["start"])) < len(c0)                                  # equal starts on one contig
    assert ((c0["start"] < 131072) & (c0["end"] >= 131072)).any()                 # across a bucket border
    assert not (f["contig"] == 2).any() and (f["is_negative_strand"] == 1).any() and (f["is_negative_strand"] == 0).any()


def test_sanitizer_program(tmp_path):
    exe = str(tmp_path / "cellassign_check")
    r = subprocess.run(ASAN_CMD + ["-o", exe, CHECK_SRC, "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for seed in ("1", "2061"):
        r = subprocess.run([exe, seed], capture_output=True, text=True)
        assert r.returncode == 0, (seed, r.stdout[-2000:], r.stderr[-4000:])
