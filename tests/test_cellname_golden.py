"""The reference's own answers on read names (tests/golden/cellname/cellname.npz, made by
make_cellname_golden.py with cellCounts_scan_read_name_str, cellCounts_get_sample_id and the two
hamming_dist_ATGC_max1 functions): the classes of names it holds, counted from the file alone, and the
plain-C model (tests/native/cellname_model.c) equal to it on every byte."""
import numpy as np
import pytest

from tests.cellname_common import (CLASSES, LINES, MODES, ROWS, class_counts, fixture_names, load_fixture, make_names, model_lib,
                                   model_parse, row_text_array)

CLASS_BAR = 20


def test_fixture_holds_every_class():
    z, total = load_fixture(), dict.fromkeys(CLASSES, 0)
    for which, (mode, bl, ul) in MODES.items():
        names, ref = fixture_names(which), z[which + "_ref"]
        assert len(names) == len(ref) >= 1025
        for k, v in class_counts(names, mode, ref[:, 2], ref[:, 3]).items():
            total[k] += v
    for k in CLASSES:
        assert total[k] >= CLASS_BAR, (k, total[k])
    # the sheet and the names are the ones the tests compose
    assert (z["rows_text"] == row_text_array()).all() and z["rows_lane"].tolist() == [r[0] for r in ROWS]
    assert z["rows_sample"].tolist() == [r[1] for r in ROWS] and z["lines"].tolist() == LINES
    assert fixture_names("bcl")[:50] == make_names("bcl", 1658)[:50]


@pytest.mark.parametrize("which", list(MODES))
def test_model_equals_the_reference(which):
    mode, bl, ul = MODES[which]
    z, names = load_fixture(), fixture_names(which)
    m, ref = model_parse(names, mode, bl, ul, threads=3), z[which + "_ref"]
    assert (m["status"] == 0).all()                     # the fixture holds names of the reference's contract only
    for col, k in enumerate(("fields", "trimmed_len", "lane", "sample_no")):
        assert (m[k] == ref[:, col]).all(), k
    assert (m["bc"] == z[which + "_bc"]).all() and (m["umi"] == z[which + "_umi"]).all()
    assert set(np.unique(ref[:, 3])) >= {-1, 1, 2, 3, 4, 5, 6, 7, 8}


def test_model_hamming_equals_the_reference():
    z, M = load_fixture(), model_lib()
    for (a, b), (d1, d2) in zip(z["pairs"], z["pair_dist"]):
        ta, tb = a.tobytes().split(b"\0")[0], b.tobytes().split(b"\0")[0]
        assert M.cellname_max1(ta, tb) == d1 and M.cellname_max1_2p(ta, tb) == d2
    d = z["pair_dist"]
    assert (d[:, 0] == 0).sum() >= 20 and (d[:, 0] == 1).sum() >= 20 and (d[:, 0] == 999).sum() >= 20
    assert (d[:, 1] == 2).sum() >= 20 and (d[:, 1] == 999).sum() >= 20
