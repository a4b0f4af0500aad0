"""The reference-made golden of fragile junction voting (tests/golden/fragile/fragile.npz, made by
tests/golden/fragile/make_fragile_golden.py from oracle/ref_dump_hook.c's SVG_REF_FRAGILE dump) and
the comparison of a (windows, slots) result -- the oracle's or the GPU's -- with it."""
import json
import os

import numpy as np

from subread_amd.abi import FRAGILE_SLOT_DTYPE, ReadBatch, default_params, PROGRAM_SUBJUNC
from tests.common import GOLD, VtReads

# svg_ref_fwin / svg_ref_fslot of oracle/ref_dump_hook.c
REF_WIN_DTYPE = np.dtype([("call", "<u4"), ("window", "<u2"), ("full_rl", "<u2"), ("negative_strand", "u1"),
                          ("junction", "u1"), ("event_negative", "u1"), ("pad", "u1"), ("low_border", "<u4"),
                          ("high_border", "<u4"), ("small_side", "<u4"), ("large_side", "<u4"), ("max_vote", "<i2"),
                          ("n_used", "<u2"), ("start", "<u2"), ("length", "<u2"), ("items", "<u2", (30,))])
REF_SLOT_DTYPE = np.dtype([("pos", "<u4"), ("votes", "<i2"), ("coverage_start", "<i2"), ("coverage_end", "<i2"),
                           ("rec", "<i2", (9,))])
assert REF_WIN_DTYPE.itemsize == 96 and REF_SLOT_DTYPE.itemsize == 28

GOLDEN_SETS = ("fredge_full_se", "fredge_full_pe", "fredge_gapped_se", "fredge_gapped_pe")
PE_LENGTHS = (161, 181, 241, 700)   # the pe sets; the two ends of a pair differ in length (fredge_reads)
AMBIGUOUS_CAP = 0.02   # junction windows whose large side the dump could not tell: the maker's cap
UNKNOWN = 0xffffffff


class FragileGolden:
    """one read set of the golden: reads (VtReads), params, w (REF_WIN_DTYPE per window), s
    (REF_SLOT_DTYPE, every used slot window by window), first (w's first slot in s)"""

    def __init__(self, z, name):
        self.name = name
        self.key = name.rsplit("_", 1)[0]

        def batch(e):
            return ReadBatch(z["%s.%s_seq" % (name, e)], z["%s.%s_off" % (name, e)], z["%s.%s_len" % (name, e)])

        self.reads = VtReads.__new__(VtReads)
        self.reads.r1 = batch("r1")
        self.reads.r2 = batch("r2") if name + ".r2_seq" in z else None
        self.reads.cls = z[name + ".cls"].astype(str)
        self.reads.strand = z[name + ".strand"]
        self.params = default_params(PROGRAM_SUBJUNC, self.reads.r2 is not None)
        n = len(z[name + ".w.call"])
        self.w = np.zeros(n, REF_WIN_DTYPE)
        for f in REF_WIN_DTYPE.names:
            self.w[f] = z["%s.w.%s" % (name, f)]
        self.s = np.zeros(int(self.w["n_used"].sum()), REF_SLOT_DTYPE)
        for f in REF_SLOT_DTYPE.names:
            self.s[f] = z["%s.s.%s" % (name, f)].T
        self.first = np.concatenate([[0], np.cumsum(self.w["n_used"].astype(np.int64))])

    def table(self, i):
        return self.s[self.first[i]:self.first[i + 1]]


_golden = {}


def fragile_golden(name):
    if not _golden:
        z = np.load(os.path.join(GOLD, "fragile", "fragile.npz"), allow_pickle=False)
        _golden["note"] = json.loads(str(z["note"]))
        for n in GOLDEN_SETS:
            _golden[n] = FragileGolden(z, n)
    return _golden[name]


def expected_slots(g):
    """the reported slots of every window, from the reference's dumped tables by the plain filter
    votes >= max_vote and rec[3] != 0 in row-major order, rec[7..8] zeroed where rec[6] == 0
    -> (n_slots per window, FRAGILE_SLOT_DTYPE)"""
    win = np.repeat(np.arange(len(g.w)), g.w["n_used"])
    keep = (g.s["votes"] >= g.w["max_vote"][win]) & (g.s["rec"][:, 3] != 0)
    out = np.zeros(int(keep.sum()), FRAGILE_SLOT_DTYPE)
    out["position"] = g.s["pos"][keep]
    out["rec"] = g.s["rec"][keep]
    out["rec"][out["rec"][:, 6] == 0, 7:] = 0
    return np.bincount(win[keep], minlength=len(g.w)), out


def assert_equals_reference(got, g):
    """(windows, slots) of OracleIndex.fragile / VoteIndex.fragile on g's reads against the
    reference's dump: start, length, junction, small_side, large_side and gtag (the last two where
    the dump knows them), n_slots and the slots"""
    gw, gs = got
    w = g.w
    assert len(gw) == len(w), (len(gw), len(w))
    # the dump's (call, window) order is the result's (block, read, strand, end, window) order
    assert (gw["strand"] == w["negative_strand"]).all() and (gw["window"] == w["window"]).all()
    call = np.concatenate([[0], np.cumsum((gw["window"] == 0)[1:])])
    assert (call == w["call"]).all()

    def same(field, a, b, mask=None):
        bad = np.flatnonzero((a != b) & (True if mask is None else mask))
        assert not len(bad), "%s: %d windows differ from the reference, first: window %d (read %d strand %d end %d " \
            "window %d, class %s): %s != reference %s" % (field, len(bad), bad[0], gw["read"][bad[0]], gw["strand"][bad[0]],
                                                          gw["end"][bad[0]], gw["window"][bad[0]],
                                                          g.reads.cls[gw["read"][bad[0]]], a[bad[0]], b[bad[0]])

    same("start", gw["start"], w["start"])
    same("length", gw["length"], w["length"])
    same("junction", gw["junction"], w["junction"])
    j = w["junction"] == 1
    same("small_side", gw["small_side"], w["small_side"], j)
    known = j & (w["large_side"] != UNKNOWN)
    same("large_side", gw["large_side"], w["large_side"], known)
    same("gtag", gw["gtag"], 1 - w["event_negative"].astype(np.int64), known)
    n, want = expected_slots(g)
    same("n_slots", gw["n_slots"], n)
    assert len(gs) == len(want), (len(gs), len(want))
    first = np.concatenate([[0], np.cumsum(n)])[:-1]
    same("first_slot", gw["first_slot"], first, n > 0)
    bad = np.flatnonzero((gs["position"] != want["position"]) | (gs["rec"] != want["rec"]).any(1))
    assert not len(bad), "%d reported slots differ from the reference, first: slot %d (window %d) %s != reference %s" % (
        len(bad), bad[0], int(np.searchsorted(first, bad[0], "right")) - 1, gs[bad[0]], want[bad[0]])
