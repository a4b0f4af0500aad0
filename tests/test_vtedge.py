"""CPU: the vtedge fixtures (tests/common.py vtedge_*, tests/golden/*_vtedge*) reach the edges they
are there for.  Everything here is derived with numpy from the genome's and the reads' bases alone:
exact occurrences of a read's 16-mers, grouped the way the vote table groups them (row
(position / 5) % 30, 24 slots per row; a subread at read offset `off` found at genome position
`pos` votes for pos - off).  These are conditions on the inputs: if one fails, the genome or the
read generator is wrong, not the limit."""
import numpy as np
import pytest

from tests.common import (GOLD, VTEDGE_EDGE_COPIES, VTEDGE_LADDER, VTEDGE_MS, VTEDGE_R155, VTEDGE_T150,
                          VTEDGE_THR, ensure_built, revcomp_bytes, vtedge_layout)

ensure_built()

ROWS, SEG, SPACE = 30, 5, 24
THRESHOLD = 100          # subread-buildindex -f: 16-mers found this often or more are left out
SE_CASES = ["se_full_vtedge", "se_gapped_vtedge", "se_full_vtedge_I16", "se_mb_vtedge_fullM1"]
SE161_CASES = ["se_full_vtedge_161", "se_gapped_vtedge_161"]
PE_CASES = ["pe_full_vtedge", "pe_gapped_vtedge"]
SJ_CASES = ["sj_se_full_vtedge", "sj_pe_gapped_vtedge"]
CODE = np.full(256, 255, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    CODE[_c] = _i


def pack16(seq):
    """the 16-mers of seq as integers (4 for a 16-mer with a base other than ACGT)"""
    c = CODE[np.asarray(seq, np.uint8)].astype(np.uint64)
    n = len(c) - 15
    if n <= 0:
        return np.zeros(0, np.uint64)
    k = np.zeros(n, np.uint64)
    bad = np.zeros(n, bool)
    for j in range(16):
        k = (k << np.uint64(2)) | (c[j:j + n] & np.uint64(3))
        bad |= c[j:j + n] == 255
    k[bad] = np.uint64(1) << np.uint64(40)
    return k


class Kmers:
    """every 16-mer of the genome (none across a contig border) -> its positions in the
    concatenated genome"""

    def __init__(self, g):
        keys, pos = [], []
        for s, st in zip(g.seqs, g.starts):
            k = pack16(s)
            keys.append(k)
            pos.append(int(st) + np.arange(len(k), dtype=np.int64))
        keys, pos = np.concatenate(keys), np.concatenate(pos)
        o = np.argsort(keys, kind="stable")
        self.keys, self.pos = keys[o], pos[o]

    def find(self, k):
        a, b = np.searchsorted(self.keys, k, "left"), np.searchsorted(self.keys, k, "right")
        return self.pos[a:b]

    def votes(self, read, offsets=None):
        """[(offset, positions)] of the read's 16-mers"""
        ks = pack16(read)
        return [(off, self.find(ks[off])) for off in (range(len(ks)) if offsets is None else offsets)]


@pytest.fixture(scope="module")
def km():
    return Kmers(vtedge_layout()[0])


class Tagged:
    def __init__(self, name):
        z = np.load("%s/%s.npz" % (GOLD, name), allow_pickle=False)
        self.n = len(z["r1_len"])
        self.z = z
        self.cls, self.exact, self.strand = z["cls"], z["exact"], z["strand"]

    def read(self, i, end=1):
        o, l = self.z["r%d_off" % end], self.z["r%d_len" % end]
        return self.z["r%d_seq" % end][int(o[i]):int(o[i]) + int(l[i])]

    def source(self, i):
        """read i as it lies on the genome's forward strand"""
        r = self.read(i)
        return revcomp_bytes(r) if self.strand[i] else r

    def of(self, cls, exact_only=True):
        return [int(i) for i in np.flatnonzero((self.cls == cls) & (self.exact | (not exact_only)))]


@pytest.mark.parametrize("name", SE_CASES + SE161_CASES + PE_CASES + SJ_CASES)
def test_every_class_has_30_reads(name):
    """(The per-class checks below count the exact half of a class, so they ask for 10 of them; the
    30 is asserted here on the whole class.)"""
    t = Tagged(name)
    assert t.n <= 2200
    cls, cnt = np.unique(t.cls, return_counts=True)
    assert cnt.min() >= 30, dict(zip(cls, cnt))
    want = set()
    if name in SE_CASES:
        ladder = (18, 19, 20, 21) if "gapped" in name else (16, 17, 18, 19)
        want = set(["t150_%d" % n for n in VTEDGE_T150] + ["r155_%d" % n for n in VTEDGE_R155] + ["r145_40"] +
                   ["ms_%d" % p for p in VTEDGE_MS] + ["thr_%d" % n for n in VTEDGE_THR] +
                   ["edge_first", "edge_last", "bnd_first", "bnd_last", "l160_t150_40", "l160_r145_40", "l160_r155_80"] +
                   ["lad%d_%d" % (L, n) for L in ladder for n in VTEDGE_LADDER])
        if name.endswith("M1"):
            want |= set(["cs%d_%d" % (k, p) for k in (2, 3) for p in (2, 3, 20)] +
                        ["ce%d_%d" % (k, p) for k in (1, 2) for p in (2, 3, 20)] + ["blkhigh"])
        if name.endswith("I16"):
            assert (t.z["r1_len"] == 161).sum() >= 30
        else:
            assert t.z["r1_len"].max() == 160      # one longer read would take the batch off the lane kernels
    elif name in SE161_CASES:
        want = {"l160_t150_40", "l160_r145_40", "l160_r155_80"}
        assert set(np.unique(t.z["r1_len"])) == {160, 161} and (t.z["r1_len"] == 161).sum() >= 30
    elif name in PE_CASES:
        want = set(["pe_r155_%d_fl" % n for n in (63, 64, 65, 80)] + ["pe_fl_r155_%d" % n for n in (63, 64, 65, 80)] +
                   ["pe_t150_%d" % n for n in (24, 25, 40)])
    else:
        want = set("sj%d_%s" % (L, a) for L in (100, 200) for a in ("t150_25", "t150_40", "r155_20", "r155_65"))
        assert any(c.startswith("sj100_ms_") for c in cls) and any(c.startswith("sj200_ms_") for c in cls)
    assert want <= set(cls), sorted(want - set(cls))


def fullest_row(km, read):
    """the most votes any 16-mer of the read puts into one row of the table"""
    best = 0
    for off, pos in km.votes(read):
        if len(pos):
            best = max(best, int(np.bincount(((pos - off) // SEG) % ROWS, minlength=ROWS).max()))
    return best


@pytest.mark.parametrize("name", SE_CASES)
def test_same_row_arrays_fill_a_row(name, km):
    """150 = 5 * 30: the n copies of a 16-mer of a t150_<n> array vote into one row.  23 and 24
    stay within the row's 24 slots, 25 / 26 / 30 / 40 go past them."""
    t = Tagged(name)
    for cls, n in [("t150_%d" % n, n) for n in VTEDGE_T150] + [("edge_first", VTEDGE_EDGE_COPIES),
                                                              ("edge_last", VTEDGE_EDGE_COPIES)]:
        ids = t.of(cls)
        assert len(ids) >= 10
        for i in ids:
            full = fullest_row(km, t.source(i))
            assert full == n, (cls, i, full)
            assert (full > SPACE) == (n > SPACE)
    assert SPACE in VTEDGE_T150 and SPACE - 1 in VTEDGE_T150 and SPACE + 1 in VTEDGE_T150


@pytest.mark.parametrize("name", SE_CASES)
def test_ladder_reads_have_exact_candidate_and_slot_counts(name, km):
    """A lad<L>_<n> read lies inside one 155-bp unit of an n-copy array.  At gap 1 its subreads are
    the offsets 0 .. L-16: (L - 15) * n candidates on its own strand, n distinct positions more than
    16 bases apart (n slots), nothing on the other strand.  (These are counts in the genome: the full index
    holds every one of them, a gapped index every third; its case has 18..21-bp reads.)"""
    t = Tagged(name)
    seen = set()
    for cls in sorted(set(c for c in t.cls if c.startswith("lad"))):
        L, n = int(cls[3:5]), int(cls.split("_")[1])
        ids = t.of(cls)
        assert len(ids) >= 30
        for i in ids:
            src = t.source(i)
            assert len(src) == L
            v = km.votes(src)
            assert len(v) == L - 15
            assert sum(len(p) for _, p in v) == (L - 15) * n, (cls, i)
            slots = np.unique(np.concatenate([p - off for off, p in v]))
            assert len(slots) == n and np.diff(slots).min() > 16, (cls, i)
            # each copy one row further: no two of them in one row while n <= 30
            assert len(np.unique((slots // SEG) % ROWS)) == n
            assert sum(len(p) for _, p in km.votes(revcomp_bytes(src))) == 0
        seen.add((L, n))
    if "gapped" not in name:
        # the lane kernels' limits at N and N + 1: 40 candidates (17 bp: 20 / 21 copies), 16 and 20 slots
        assert {(17, 20), (17, 21), (16, 16), (16, 17), (17, 16), (17, 17), (16, 20), (16, 21)} <= seen


@pytest.mark.parametrize("name", PE_CASES)
def test_pairs_fill_more_than_64_end0_positions(name, km):
    """The array end of a pe_r155_<n>_fl / pe_fl_r155_<n> pair lies inside one unit: its 16-mers vote
    for exactly n positions, 63 / 64 / 65 / 80 -- up to and past the 64 entries of the paired wave
    kernel's compacted list; the flank end has one position."""
    t = Tagged(name)
    for n in (63, 64, 65, 80):
        for cls, arr_end in (("pe_r155_%d_fl" % n, 1), ("pe_fl_r155_%d" % n, 2)):
            ids = t.of(cls)
            assert len(ids) >= 30
            for i in ids:
                ends = {1: t.read(i, 1), 2: revcomp_bytes(t.read(i, 2))}
                if t.strand[i]:
                    ends = {1: revcomp_bytes(t.read(i, 1)), 2: t.read(i, 2)}
                a = np.unique(np.concatenate([p - off for off, p in km.votes(ends[arr_end])]))
                b = np.unique(np.concatenate([p - off for off, p in km.votes(ends[3 - arr_end])]))
                assert len(a) == n and len(b) == 1, (cls, i, len(a), len(b))
                assert (len(a) > 64) == (n > 64)
                assert 200 <= abs(int(b[0]) - int(a[np.argmin(abs(a - b[0]))])) <= 600


@pytest.mark.parametrize("name", SE_CASES)
def test_microsatellite_reads_stay_under_the_threshold_and_within_tolerance(name, km):
    """Every 16-mer of a read inside the period-p microsatellite occurs 40..95 times (vtedge_ms_copies(p),
    one more where the flank happens to continue the period; under the builder's threshold of 100), p bases apart: within the default tolerance of
    5 for p = 2, 3, 5, within -I 16's for every period but 17, which lies one base outside it."""
    t = Tagged(name)
    tol = 16 if name.endswith("I16") else 5
    inside = 0
    for p in VTEDGE_MS:
        ids = t.of("ms_%d" % p)
        assert len(ids) >= 10
        for i in ids:
            for off, pos in km.votes(t.source(i)):
                assert 40 <= len(pos) <= 95 < THRESHOLD, (p, i, off, len(pos))
                assert (np.diff(np.sort(pos)) == p).all()
        inside += p <= tol
    assert inside == (3 if tol == 5 else 7)
    assert tol + 1 in VTEDGE_MS


def test_threshold_arrays_straddle_the_repeat_threshold(km):
    """thr_<n>: a 16-mer inside the 157-bp unit occurs n times, one across two copies n - 1 times:
    99 / 98, 100 / 99 and 101 / 100, both sides of the threshold the index md5 pins down."""
    g, cons = vtedge_layout()
    for n in VTEDGE_THR:
        c = cons["thr_%d" % n]
        counts = [len(p) for _, p in km.votes(g.flat[c["flat"]:c["flat"] + 2 * 157 + 15])]
        assert set(counts) == {n, n - 1}
    assert THRESHOLD in VTEDGE_THR and THRESHOLD - 1 in VTEDGE_THR and THRESHOLD + 1 in VTEDGE_THR


@pytest.mark.parametrize("name", SE_CASES)
def test_boundary_reads_hang_over_the_genome_ends(name, km):
    """bnd_first: 20 bases that are not in the genome, then the first contig's first 80 (inside the
    edge_first array, which starts at base 0): every subread at offset >= 20 votes for 20 bases
    before the genome's first base in the first copy.  bnd_last mirrors it past the last base."""
    g, cons = vtedge_layout()
    t = Tagged(name)
    assert cons["edge_first"]["flat"] == 0 and cons["edge_last"]["flat"] + cons["edge_last"]["length"] == len(g.flat)
    for cls in ("bnd_first", "bnd_last"):
        ids = t.of(cls, exact_only=False)
        assert len(ids) >= 30 and set(t.strand[ids]) == {0, 1}
        for i in ids:
            src = t.source(i)
            assert len(src) == 100
            votes = np.concatenate([p - off for off, p in km.votes(src)])
            if cls == "bnd_first":
                assert (src[20:] == g.seqs[0][:80]).all() and votes.min() == -20
            else:
                assert (src[:80] == g.seqs[-1][-80:]).all() and votes.max() + 100 == len(g.flat) + 20
