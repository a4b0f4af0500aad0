"""The plain-C model of cellCounts' UMI stage (tests/native/cellumi_model.c) against the reference's
own answers (tests/golden/cellumi/cellumi.npz, made by make_cellumi_golden.py from the reference's
ADD_key_struct, comparator and merge steps): every byte of the entries, the count table and the
removed numbers on every case, and the classes the fixture must hold, counted from the committed
file."""
import numpy as np
import pytest

from tests.cellumi_common import FIXTURE_CASES, class_counts, fixture_case, model_run, same_result

LENGTHS = [c[0] for c in FIXTURE_CASES]


def mask_unknown(got, known):
    """the acceptor of an entry whose key in the reference's table another cell's entry took
    (cell-counts.c:3581-3587: the key holds no cell) is not in the fixture"""
    e = got["entries"].copy()
    e["acceptor_umi"][~known] = b""
    return dict(got, entries=e)


@pytest.mark.parametrize("L", LENGTHS)
def test_model_equals_the_reference(L):
    obs, want, known = fixture_case(L)
    got = model_run(*obs, L)
    same_result(mask_unknown(got, known), want)


def test_fixture_holds_every_class():
    total = {}
    for L in LENGTHS:
        obs, want, known = fixture_case(L)
        assert (obs[0] <= 0).sum() >= 20 and (obs[1] < 0).sum() >= 20 and set(np.unique(want["entries"]["sample"])) == {1, 2}
        for k, v in class_counts(want["entries"], L).items():
            total[k] = total.get(k, 0) + v
        if L > 4:
            assert known.all()       # only 4-base UMIs repeat across the cells of one gene
    for k, v in total.items():
        # one section of a few thousand entries is enough: it is what makes the file large
        assert v >= (1 if k == "thousands" else 20), (k, v, total)
    assert len(total) == 18
