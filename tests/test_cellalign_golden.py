"""svg_cell_align_batch on the CPU: the plain-C model (tests/native/cellalign_model.c) against the
fixtures the reference's own cellCounts_select_and_write_alignments wrote
(tests/golden/cellalign/, make_cellalign_golden.py), the edges those fixtures reach, and the
binding's structs against the header."""
import ctypes
import os
import re

import numpy as np
import pytest

from subread_amd import abi
from tests.cellalign_common import (CASES, EDGES, asan_check, case_params, cigar_ops, golden_case, host_index, model_align,
                                    raw)
from tests.cellvote_common import unpack_ascii
from tests.common import ROOT, IndexCache

IDS = ["%s-n%d-%s" % c for c in CASES]

# Reads per case that must reach each edge.  The bar is 20, as the issue sets it.  Lowered where the
# reference alone cannot reach it on an index:
#   - a gapped index (gap 3) with 7 or 10 subreads: a subread votes only where its offset meets the
#     index's phase, so few sections are voted.  An indel shows in the CIGAR only when the sections
#     on both of its sides were voted, which about one read with an indel in ten manages, and two
#     indels (three voted sections) next to never.  The bar for one indel is 10 there, and there is
#     none for two.
#   - a gapped index with 7 subreads, tied top scores: two or three subreads of a read can vote
#     there, min_votes_per_mapped_read is 3, and a third of the reads map at all (264 and 330 of
#     1090); a tie needs two places that both collect three votes.  The bar is 5.
#   - a candidate scored 0 for rebuilt_rlen != read_len, every index: the pieces of the CIGAR sum to
#     the read length by construction unless one of their numbers is negative (reduce_Cigar reads
#     "-3M" as 1 '-' and 3 M), which needs a section that starts before the previous one's correct
#     base.  The reference reached it for 2 of the 15,260 reads of all cases.  No bar per case; the
#     model counts it, the count is printed by the generator, and test_rebuilt_rlen_is_reached asks
#     that all cases together reach it at least once.
BAR = 20


def bar_of(key, total, edge):
    if "gapped" in key and total < 20:
        if edge in ("insertion", "deletion"):
            return 10
        if edge == "two_indels":
            return 0
    if "gapped" in key and total == 7 and edge == "tie":
        return 5
    if edge == "zero_rlen":
        return 0
    return BAR


@pytest.fixture(scope="module")
def cache(tmp_path_factory):
    return IndexCache(str(tmp_path_factory.mktemp("cellalign_ix")))


@pytest.fixture(scope="module")
def hosts(cache):
    return {k: host_index(cache.get(k)) for k in sorted(set(c[0] for c in CASES))}


@pytest.mark.parametrize("key,total,which", CASES, ids=IDS)
def test_model_equals_reference(hosts, key, total, which):
    pk, ea, eb, heads, alns = golden_case(key, total, which)
    got = model_align(hosts[key], unpack_ascii(pk), (ea, eb), **case_params(total, which))
    assert got is not None
    assert (raw(got[0]) == raw(heads)).all()
    assert len(got[1]) == len(alns) and (raw(got[1]) == raw(alns)).all()


def edge_counts(heads, alns):
    ops = cigar_ops(alns)
    cig = [c.decode() for c in alns["cigar"]]
    read_of = np.repeat(np.arange(len(heads)), heads["n_records"])

    def reads(mask):
        return len(np.unique(read_of[np.asarray(mask, bool)]))

    # the weight is a factor of the score: 10^7 (a base in an exon), else 13 or 10
    sc = alns["score"]
    top = sc >= 10 ** 12   # below: at most 160 * 10^6 * 13; an exon's: at least 40 * 10^6 / 11 * 10^7
    return {
        "head_clip": reads([re.match(r"^\d+S", c) is not None for c in cig]),
        "tail_clip": reads([c.endswith("S") for c in cig]),
        "insertion": reads(["I" in o for o in ops]),
        "deletion": reads(["D" in o for o in ops]),
        "two_indels": reads([len(re.findall(r"[ID]", c)) >= 2 for c in cig]),
        "reverse": reads(alns["flags"] == 16),
        "exon": reads(top),
        "unmapped": int((heads["n_records"] == 0).sum()),
        "multi": int((heads["n_records"] > 1).sum()),
    }


@pytest.fixture(scope="module")
def model_edges(hosts):
    """per case, once: the model's (heads, alns, EDGE_* bits per read) on the fixture's reads"""
    out = {}

    def get(key, total, which):
        if (key, total, which) not in out:
            pk, ea, eb, _, _ = golden_case(key, total, which)
            out[key, total, which] = model_align(hosts[key], unpack_ascii(pk), (ea, eb), want_edges=True,
                                                 **case_params(total, which))
        return out[key, total, which]

    return get


@pytest.mark.parametrize("key,total,which", CASES, ids=IDS)
def test_fixture_edges(hosts, model_edges, key, total, which):
    """the edges the records show, and those only the model sees per candidate (a candidate scored 0
    for its mismatches or for rebuilt_rlen, tied top scores, weight 13): its records are the
    fixture's (test_model_equals_reference), so its candidates are the reference's"""
    pk, ea, eb, heads, alns = golden_case(key, total, which)
    e = edge_counts(heads, alns)
    mh, ma, bits = model_edges(key, total, which)
    assert (raw(mh) == raw(heads)).all() and (raw(ma) == raw(alns)).all()
    e.update({k: int(((bits & v) != 0).sum()) for k, v in EDGES.items()})
    assert e["weight_top"] >= e["exon"]
    print(key, total, which, e)
    for k in ("head_clip", "tail_clip", "insertion", "deletion", "two_indels", "reverse", "exon", "unmapped", "zero_mm",
              "zero_rlen", "tie", "weight13", "weight_top"):
        assert e[k] >= bar_of(key, total, k), (k, e)
    if which == "second":
        assert e["multi"] >= BAR, e


def test_rebuilt_rlen_is_reached(model_edges):
    """the zero_rlen bar is 0 on every case (bar_of), which asserts nothing on its own: over all
    cases together at least one read has a candidate scored 0 for rebuilt_rlen != read_len, so
    that regenerated fixtures cannot lose that path unnoticed"""
    n = sum(int(((model_edges(*c)[2] & EDGES["zero_rlen"]) != 0).sum()) for c in CASES)
    print("zero_rlen over all cases", n)
    assert n >= 1


def test_model_clean_under_sanitizers(hosts, tmp_path):
    """tests/native/cellalign_check.c (its own main: the model over a case written to a flat file,
    compared with the expected records) built -fsanitize=address,undefined and run as a program of
    its own on every case"""
    asan_check(hosts, str(tmp_path))


def test_structs_match_header():
    src = open(os.path.join(ROOT, "include", "subread_vote.h")).read()
    body = re.search(r"typedef struct svg_cell_align_params \{(.*?)\} svg_cell_align_params;", src, re.S).group(1)
    names = re.findall(r"int32_t\s+(\w+);", body)
    assert names == [k for k, _ in abi.SvgCellAlignParams._fields_]
    assert ctypes.sizeof(abi.SvgCellAlignParams) == 4 * len(names)
    body = re.search(r"typedef struct svg_cell_aln \{(.*?)\} svg_cell_aln;", src, re.S).group(1)
    assert re.findall(r"(\w+)(?:\[\w+\])?;", body) == [n for n in abi.CELL_ALN_DTYPE.names]
    body = re.search(r"typedef struct svg_cell_aln_head \{(.*?)\} svg_cell_aln_head;", src, re.S).group(1)
    assert re.findall(r"(\w+);", body) == [n for n in abi.CELL_ALN_HEAD_DTYPE.names]
    assert int(re.search(r"#define SVG_CELL_CIGAR\s+(\d+)", src).group(1)) == abi.CELL_CIGAR
    assert abi.CELL_ALN_DTYPE.itemsize == 128 and abi.CELL_ALN_HEAD_DTYPE.itemsize == 16
    assert abi.CELL_ALN_DTYPE.fields["cigar"][1] == 20


def test_model_refuses_what_the_library_refuses(hosts):
    key = CASES[0][0]
    pk = golden_case(*CASES[0])[0]
    b = unpack_ascii(pk).slice(0, 4)
    for bad in (dict(total_subreads=6), dict(total_subreads=21), dict(max_indel_length=4), dict(min_votes_per_mapped_read=0),
                dict(min_votes_per_mapped_read=65), dict(max_differential_from_top_vote_number=0),
                dict(max_differential_from_top_vote_number=31), dict(max_mismatching_bases_in_reads=-1),
                dict(max_mismatching_bases_in_reads=101), dict(min_mapped_length_for_mapped_read=-2),
                dict(min_mapped_length_for_mapped_read=161), dict(max_reported_alignments_per_read=0),
                dict(max_reported_alignments_per_read=31)):
        assert model_align(hosts[key], b, **bad) is None, bad
