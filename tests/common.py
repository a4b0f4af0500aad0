"""Shared helpers for the parity tests: golden fixtures, index cache, record comparison."""
import glob
import gzip
import hashlib
import json
import os
import re
import subprocess

import numpy as np

from subread_amd.abi import (MAPPING_DTYPE, SUBJUNC_DTYPE, ReadBatch, SvgParams, PROGRAM_ALIGN,
                             PROGRAM_SUBJUNC)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def ensure_built():
    """Build the product library and the oracle restatement if missing (CPU-only compile)."""
    lib = os.path.join(ROOT, "subread_amd", "lib", "libsubread_amd.so")
    if not os.path.exists(lib):
        subprocess.run(["make", "-C", os.path.join(ROOT, "subread_amd", "csrc"), "-j8"], check=True,
                       capture_output=True)
    olib = os.path.join(ROOT, "oracle", "lib", "libsvoracle.so")
    if not os.path.exists(olib):
        subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "port"], check=True, capture_output=True)


def golden_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLD, "*.npz")))


def index_md5():
    with open(os.path.join(GOLD, "index_md5.json")) as f:
        return json.load(f)


def md5(p):
    h = hashlib.md5()
    with open(p, "rb") as f:
        for blk in iter(lambda: f.read(1 << 24), b""):
            h.update(blk)
    return h.hexdigest()


# seeded synthetic genomes: lengths, seed (repeats 2500 copies of 300-bp elements, 16 families, 4%)
SYNTH_GENOMES = {
    "synth4242": ([300000, 250000, 17, 200000, 120000], 4242),
    # one 3 Mbp contig: a -M 17 / -M 6 build splits it deep inside (read_len > MIN_READ_SPLICING),
    # so consecutive blocks overlap by ~2 Mbp
    "long777": ([3000000, 150000, 900000], 777),
}


# sublong's vote table has 64973 rows of 51 slots: 54 copies of one element exactly 64973 bases
# apart put 54 positions of every subread of it in the same row (LRMsorted-hashtable.c:503-514)
LR_ROWS = 64973


def lrrow54_genome():
    from subread_amd.sim import Genome, random_genome
    g = random_genome([54 * LR_ROWS + 5000, 200000], 5454)
    a = g.seqs[0].copy()
    elem = random_genome([2000], 5455).seqs[0]
    for j in range(54):
        a[j * LR_ROWS + 1000:j * LR_ROWS + 3000] = elem
    return Genome(g.names, [a, g.seqs[1]])


# ---- vtedge: a genome built to reach the edges of the short-read vote table (gene_vote_t: 30 rows
# of 24 slots, row (kv / 5) % 30; sorted-hashtable.c:937-1123) and of the lane kernels' limits.
# Constructs, each with its own random unit, a VTEDGE_GAP of i.i.d. sequence apart:
#   t150_<n>   tandem array of n copies of a 150-bp unit (150 = 5 * 30: every copy in one row)
#   r155_<n>   unit 155: each copy one row further, copies further apart than any tolerance
#   r145_40    unit 145: one row back per copy
#   ms_<p>     microsatellite of period p, every 16-mer vtedge_ms_copies(p) times
#   thr_<n>    unit 157, n = 99 / 100 / 101 copies: both sides of the builder's repeat threshold
#   edge_first / edge_last   150-bp-unit arrays flush against the first contig's start and the
#              last contig's end
VTEDGE_CONTIGS = [160000, 120000, 100000]
VTEDGE_SEED = 2424
VTEDGE_GAP = 2000
VTEDGE_T150 = (23, 24, 25, 26, 40)
VTEDGE_R155 = (15, 16, 17, 19, 20, 21, 63, 64, 65, 80)
VTEDGE_LADDER = (15, 16, 17, 19, 20, 21)
VTEDGE_MS = (2, 3, 5, 6, 7, 11, 16, 17)
VTEDGE_THR = (99, 100, 101)
VTEDGE_EDGE_COPIES = 30
VTEDGE_BLOCK0_OVER = 1226   # bases of chr2 in the first block of the -F -M 1 index (blocks 0..164840, 163614..)
_COMP = np.full(256, ord("N"), np.uint8)
for _a, _b in (("A", "T"), ("C", "G"), ("G", "C"), ("T", "A")):
    _COMP[ord(_a)] = ord(_b)
_ACGT = np.frombuffer(b"ACGT", np.uint8)


def vtedge_ms_copies(p):
    """occurrences of every 16-mer of the period-p microsatellite (its length is p * copies + 15)"""
    return 90 if p <= 5 else 60


def revcomp_bytes(a):
    return _COMP[np.asarray(a, np.uint8)[::-1]]


_vtedge_cache = []


def vtedge_layout():
    """-> (Genome, constructs): constructs maps a name to dict(contig, start (in the contig), flat
    (start in the concatenated genome), unit, copies, length)."""
    if _vtedge_cache:
        return _vtedge_cache[0]
    from subread_amd.sim import Genome, random_genome
    g = random_genome(VTEDGE_CONTIGS, VTEDGE_SEED)
    seqs = [s.copy() for s in g.seqs]
    rng = np.random.default_rng(VTEDGE_SEED)
    todo = [("edge_first", 150, VTEDGE_EDGE_COPIES)]
    todo += [("t150_%d" % n, 150, n) for n in VTEDGE_T150]
    todo += [("r155_%d" % n, 155, n) for n in VTEDGE_R155]
    todo += [("r145_40", 145, 40)]
    todo += [("ms_%d" % p, p, 0) for p in VTEDGE_MS]
    todo += [("thr_%d" % n, 157, n) for n in VTEDGE_THR]
    cons = {}
    ctg, cur = 0, 0
    for name, ulen, copies in todo:
        while True:
            unit = _ACGT[rng.integers(0, 4, ulen)]
            # a microsatellite unit must not itself be a repeat of a shorter one
            if not any(ulen % d == 0 and (unit == np.tile(unit[:d], ulen // d)).all() for d in range(1, ulen)):
                break
        if copies:
            body = np.tile(unit, copies)
        else:
            body = np.tile(unit, vtedge_ms_copies(ulen) + 16 // ulen + 2)[:ulen * vtedge_ms_copies(ulen) + 15]
        reserve = VTEDGE_GAP + (150 * VTEDGE_EDGE_COPIES if ctg == len(seqs) - 1 else 0)
        if cur + len(body) + reserve > len(seqs[ctg]):
            ctg, cur = ctg + 1, VTEDGE_GAP
        assert cur + len(body) + reserve <= len(seqs[ctg]), name
        seqs[ctg][cur:cur + len(body)] = body
        cons[name] = dict(contig=ctg, start=cur, unit=ulen, copies=copies, length=len(body))
        cur += len(body) + VTEDGE_GAP
    unit = _ACGT[rng.integers(0, 4, 150)]
    last = len(seqs) - 1
    body = np.tile(unit, VTEDGE_EDGE_COPIES)
    seqs[last][len(seqs[last]) - len(body):] = body
    cons["edge_last"] = dict(contig=last, start=len(seqs[last]) - len(body), unit=150, copies=VTEDGE_EDGE_COPIES,
                             length=len(body))
    g = Genome(g.names, seqs)
    for c in cons.values():
        c["flat"] = int(g.starts[c["contig"]]) + c["start"]
    _vtedge_cache.append((g, cons))
    return _vtedge_cache[0]


def vtedge_genome():
    return vtedge_layout()[0]


def _vt_mutate(rng, seg, L):
    """1% substitutions and one 1-4 bp indel; seg holds L + 8 bases"""
    r = bytearray(np.asarray(seg, np.uint8).tobytes())
    at = int(rng.integers(8, L - 8)) if L > 20 else int(rng.integers(1, L - 1))
    k = int(rng.integers(1, 5))
    if rng.random() < 0.5:
        r[at:at] = _ACGT[rng.integers(0, 4, k)].tobytes()
    else:
        del r[at:at + k]
    r = np.frombuffer(bytes(r[:L]), np.uint8).copy()
    hit = rng.random(L) < 0.01
    r[hit] = _ACGT[rng.integers(0, 4, int(hit.sum()))]
    return r


class VtReads:
    """reads of the vtedge classes: r1, r2 (ReadBatch / None), cls (class tag per read), exact
    (no substitution or indel), strand (1: the read is the reverse complement of its source)"""

    def __init__(self, s1, s2, cls, exact, strand):
        self.r1 = ReadBatch.from_list([bytes(x) for x in s1])
        self.r2 = ReadBatch.from_list([bytes(x) for x in s2]) if s2 is not None else None
        self.cls = np.array(cls)
        self.exact = np.array(exact, bool)
        self.strand = np.array(strand, np.uint8)

    def select(self, keep):
        idx = np.flatnonzero(keep)
        return VtReads([self.r1.read(int(i)) for i in idx],
                       [self.r2.read(int(i)) for i in idx] if self.r2 is not None else None,
                       self.cls[idx], self.exact[idx], self.strand[idx])


def _vt_finish(rng, rows, paired):
    order = rng.permutation(len(rows))
    rows = [rows[i] for i in order]
    return VtReads([r[0].tobytes() for r in rows], [r[1].tobytes() for r in rows] if paired else None,
                   [r[2] for r in rows], [r[3] for r in rows], [r[4] for r in rows])


def vtedge_se_reads(per, seed, with_161=False, ladder=(16, 17, 18, 19), block_bounds=False):
    """`per` reads of every single-end class, in a seeded random order.
      <array>        100- and 150-bp reads inside each array / microsatellite: half exact, half
                     with 1% substitutions and one 1-4 bp indel, both strands
      lad<L>_<n>     exact L = 16..19 bp reads inside one unit of the r155_<n> array (every 16-mer of
                     the read n times in the genome): at gap 1 a read has L - 15 subreads, so
                     (L - 15) * n candidates and n slots on its own strand.  A gapped index takes
                     ladder=(18, 19, 20, 21): there the reference reads past the end of a read
                     shorter than 18 bases, which is outside what this project reproduces
      l160_<array>   160-bp (with_161: 160- and 161-bp) reads in the 40-copy arrays
      bnd_first / bnd_last   20 random bases + the first 80 of the first contig / the last 80 of
                     the last contig + 20 random bases
    block_bounds adds the classes for a multi-block index (-F -M 1 puts the second block's first
    base at chr2's first base; its low border is that position rounded down to a multiple of 4,
    2 bases before it; the first block runs VTEDGE_BLOCK0_OVER bases into chr2):
      cs<k>_<p>      p random bases + the first 100 - p of contig k (k = 2, 3; p = 2, 3, 20): the
                     subreads past the prefix vote for p bases before the contig, on the low
                     border (p = 2) and below it (p = 3, 20) where a block starts there
      ce<k>_<p>      the mirror image at the end of contig k (k = 1, 2)
      blkhigh        exact 100-bp reads of chr2 starting VTEDGE_BLOCK0_OVER - 100 +- 25 bases in:
                     at and past the first block's high border (block end - read length)"""
    g, cons = vtedge_layout()
    rng = np.random.default_rng(seed)
    f = g.flat
    rows = []

    def emit(src, cls, exact):
        st = int(rng.random() < 0.5)
        rows.append((revcomp_bytes(src) if st else np.asarray(src, np.uint8), None, cls, exact, st))

    def inside(c, cls, lengths, i):
        L = int(lengths[i % len(lengths)])
        s = c["flat"] + int(rng.integers(0, c["length"] - L - 8))
        if (i // len(lengths)) % 2 == 0:
            emit(f[s:s + L], cls, True)
        else:
            emit(_vt_mutate(rng, f[s:s + L + 8], L), cls, False)

    for name, c in cons.items():
        for i in range(per):
            inside(c, name, (100, 150), i)
    for n in VTEDGE_LADDER:
        c = cons["r155_%d" % n]
        for L in ladder:
            for i in range(per):
                s = c["flat"] + 155 * int(rng.integers(0, n)) + int(rng.integers(0, 155 - L + 1))
                emit(f[s:s + L], "lad%d_%d" % (L, n), True)
    for name in ("t150_40", "r155_80", "r145_40"):
        for i in range(per):
            inside(cons[name], "l160_" + name, (160, 161) if with_161 else (160,), i)
    first, last = g.seqs[0], g.seqs[-1]
    for i in range(per):
        emit(np.concatenate([_ACGT[rng.integers(0, 4, 20)], first[:80]]), "bnd_first", False)
        emit(np.concatenate([last[-80:], _ACGT[rng.integers(0, 4, 20)]]), "bnd_last", False)
    if block_bounds:
        for p in (2, 3, 20):
            for i in range(per):
                for k in (1, 2):
                    emit(np.concatenate([_ACGT[rng.integers(0, 4, p)], g.seqs[k][:100 - p]]), "cs%d_%d" % (k + 1, p), False)
                    emit(np.concatenate([g.seqs[k - 1][p - 100:], _ACGT[rng.integers(0, 4, p)]]), "ce%d_%d" % (k, p), False)
        for i in range(per):
            s = VTEDGE_BLOCK0_OVER - 100 + int(rng.integers(-25, 26))
            emit(g.seqs[1][s:s + 100], "blkhigh", True)
    return _vt_finish(rng, rows, False)


def vtedge_pe_reads(per, seed):
    """`per` pairs of every paired class (R2 the reverse complement of its source, -S fr):
      pe_r155_<n>_fl   R1 100 bp inside one unit of the r155_<n> array (n = 63, 64, 65, 80: n
                       distinct end-0 positions), R2 in the unique flank 200-400 bp past the array
      pe_fl_r155_<n>   the other way round: R1 in the flank before the array, R2 inside it
      pe_t150_<n>      both ends in the same t150 array"""
    g, cons = vtedge_layout()
    rng = np.random.default_rng(seed)
    f = g.flat
    rows = []

    def emit(a, b, cls):
        a, b = np.asarray(a, np.uint8), revcomp_bytes(b)
        st = int(rng.random() < 0.5)
        rows.append(((b, a) if st else (a, b)) + (cls, True, st))

    for n in (63, 64, 65, 80):
        c = cons["r155_%d" % n]
        end = c["flat"] + c["length"]
        for i in range(per):
            s = c["flat"] + 155 * int(rng.integers(n - 3, n)) + int(rng.integers(0, 56))
            d = end + int(rng.integers(200, 401))
            rows.append((np.asarray(f[s:s + 100], np.uint8), revcomp_bytes(f[d:d + 100]), "pe_r155_%d_fl" % n, True, 0))
            s = c["flat"] + 155 * int(rng.integers(0, 3)) + int(rng.integers(0, 56))
            d = c["flat"] - int(rng.integers(200, 401)) - 100
            rows.append((np.asarray(f[d:d + 100], np.uint8), revcomp_bytes(f[s:s + 100]), "pe_fl_r155_%d" % n, True, 0))
    for n in (24, 25, 40):
        c = cons["t150_%d" % n]
        for i in range(per):
            L = int(rng.choice([100, 150]))
            ins = int(rng.integers(L, 600))
            s = c["flat"] + int(rng.integers(0, c["length"] - ins))
            emit(f[s:s + L], f[s + ins - L:s + ins], "pe_t150_%d" % n)
    return _vt_finish(rng, rows, True)


VTEDGE_SJ_ARRAYS = ("t150_25", "t150_40", "r155_20", "r155_65") + tuple("ms_%d" % p for p in VTEDGE_MS)


def vtedge_sj_reads(per, seed, lengths=(100, 200)):
    """`per` spliced reads per class sj<L>_<array>, simulate_spliced_reads-style: the first exon
    part ends inside the array right before a GT, the second starts in unique sequence right after
    an AG 60..20000 bases further on the same contig; 0.5% substitutions, both strands.  (A
    microsatellite whose unit holds no GT has no class.)"""
    g, cons = vtedge_layout()
    rng = np.random.default_rng(seed)
    f = g.flat
    ag_end = np.flatnonzero((f[:-1] == ord("A")) & (f[1:] == ord("G"))).astype(np.int64) + 2
    spans = sorted((c["flat"], c["flat"] + c["length"]) for c in cons.values())
    rows = []
    for L in lengths:
        for name in VTEDGE_SJ_ARRAYS:
            c = cons[name]
            seg = f[c["flat"]:c["flat"] + c["length"]]
            gt = c["flat"] + np.flatnonzero((seg[:-1] == ord("G")) & (seg[1:] == ord("T")))
            if not len(gt):
                continue
            cend = int(g.starts[c["contig"]]) + int(g.lens[c["contig"]])
            got = 0
            while got < per:
                a = int(rng.integers(20, L - 19))
                x = int(gt[rng.integers(0, len(gt))])
                if x - a < c["flat"]:
                    continue
                d = int(np.exp(rng.uniform(np.log(60), np.log(20000))))
                k = int(np.searchsorted(ag_end, x + d))
                if k >= len(ag_end):
                    continue
                y = int(ag_end[k])
                if y + (L - a) > cend or any(s0 < y + (L - a) and y < e0 for s0, e0 in spans):
                    continue
                r = np.concatenate([f[x - a:x], f[y:y + L - a]])
                hit = rng.random(L) < 0.005
                r[hit] = _ACGT[rng.integers(0, 4, int(hit.sum()))]
                st = int(rng.random() < 0.5)
                rows.append((revcomp_bytes(r) if st else r, None, "sj%d_%s" % (L, name), not hit.any(), st))
                got += 1
    return _vt_finish(rng, rows, False)


# ---- fredge: a genome built to reach the edges of fragile junction voting's vote table
# (core_fragile_junction_voting, core-junction.c:5151-5422: per ~60-base window one gene_vote_t of
# 30 rows x 24 slots filled by gehash_go_q, sorted-hashtable.c:750-927) for subjunc reads over 160
# bases.  Constructs, FREDGE_GAP of i.i.d. sequence apart:
#   edge_first / edge_last  150-bp-unit arrays of 30 / 12 copies flush against the genome's first and
#              last base (12 never fill a row, so what the high border drops there is visible)
#   t150_<n>   n = 23, 24, 25, 40 copies of a 150-bp unit: every copy's candidate in one row; 24
#              fill it, the 25th is dropped
#   r155_80    80 copies of a 155-bp unit: one row further per copy, more than 64 used slots
#   f3rows     24 copies of a 150-bp unit that starts with 44 bases of a period-7 microsatellite
#              (then random filler): a 16-mer of it recurs at shifts 0, 7, 14, 21 in every unit (96
#              times in all: under the builder's repeat threshold of 100; the one 16-mer with a
#              fifth shift is over it on a full index), 7 > the tolerance of 5 apart, so each shift
#              fills a row of its own to 24, and where the first position is 0 or 3 mod 5 three of
#              the rows are adjacent -- a candidate in the middle one scans 72 slots
FREDGE_CONTIGS = [110000, 90000, 70000]
FREDGE_SEED = 6161
FREDGE_GAP = 2000
FREDGE_T150 = (23, 24, 25, 40)
FREDGE_EDGE_COPIES = 30
FREDGE_EDGE_LAST_COPIES = 12
FREDGE_F3_COPIES = 24
FREDGE_F3_MS = 44
FREDGE_LENGTHS = (161, 179, 180, 181, 239, 240, 241, 700, 1209)
_fredge_cache = []


def fredge_layout():
    """-> (Genome, constructs), as vtedge_layout"""
    if _fredge_cache:
        return _fredge_cache[0]
    from subread_amd.sim import Genome, random_genome
    g = random_genome(FREDGE_CONTIGS, FREDGE_SEED)
    seqs = [s.copy() for s in g.seqs]
    rng = np.random.default_rng(FREDGE_SEED)

    def unit150():
        return _ACGT[rng.integers(0, 4, 150)]

    bodies = [("edge_first", np.tile(unit150(), FREDGE_EDGE_COPIES), 150, FREDGE_EDGE_COPIES)]
    bodies += [("t150_%d" % n, np.tile(unit150(), n), 150, n) for n in FREDGE_T150]
    bodies += [("r155_80", np.tile(_ACGT[rng.integers(0, 4, 155)], 80), 155, 80)]
    while True:
        ms = _ACGT[rng.integers(0, 4, 7)]
        if len(set(ms.tolist())) >= 3:
            break
    u = np.concatenate([np.tile(ms, 9)[:FREDGE_F3_MS], _ACGT[rng.integers(0, 4, 150 - FREDGE_F3_MS)]])
    bodies += [("f3rows", np.tile(u, FREDGE_F3_COPIES), 150, FREDGE_F3_COPIES)]
    cons = {}
    ctg, cur = 0, 0
    for name, body, ulen, copies in bodies:
        if cur + len(body) + FREDGE_GAP > len(seqs[ctg]) - 20000:   # the contig's second half stays unique
            ctg, cur = ctg + 1, FREDGE_GAP
        seqs[ctg][cur:cur + len(body)] = body
        cons[name] = dict(contig=ctg, start=cur, unit=ulen, copies=copies, length=len(body))
        cur += len(body) + FREDGE_GAP
    last = len(seqs) - 1
    body = np.tile(unit150(), FREDGE_EDGE_LAST_COPIES)
    seqs[last][len(seqs[last]) - len(body):] = body
    cons["edge_last"] = dict(contig=last, start=len(seqs[last]) - len(body), unit=150, copies=FREDGE_EDGE_LAST_COPIES,
                             length=len(body))
    g = Genome(g.names, seqs)
    for c in cons.values():
        c["flat"] = int(g.starts[c["contig"]]) + c["start"]
    _fredge_cache.append((g, cons))
    return _fredge_cache[0]


def fredge_genome():
    return fredge_layout()[0]


# the -F -M 1 index of fredge has two blocks: the second one's first base is chr3's first base, and
# the first block runs FREDGE_BLOCK0_OVER bases into chr3 (index positions 0..207244 and 206018..)
FREDGE_BLOCK0_OVER = 1226
FREDGE_CHARS = ("n", "lower", "iupac", "u")


def _fr_indel(rng, seg, L):
    """one 1-3 base indel at least 20 bases from either end; seg holds L + 3 bases"""
    r = bytearray(np.asarray(seg, np.uint8).tobytes())
    at = int(rng.integers(20, L - 20))
    k = int(rng.integers(1, 4))
    if rng.random() < 0.5:
        r[at:at] = _ACGT[rng.integers(0, 4, k)].tobytes()
    else:
        del r[at:at + k]
    return np.frombuffer(bytes(r[:L]), np.uint8).copy()


def _fr_chars(rng, src, kind):
    a = np.asarray(src, np.uint8).copy()
    L = len(a)
    if kind == "n":
        a[rng.integers(0, L, max(2, L // 60))] = ord("N")
    elif kind == "lower":
        s = int(rng.integers(0, L - 100))
        a[s:s + 100] |= 0x20
    elif kind == "iupac":
        pos = rng.integers(0, L, max(2, L // 60))
        a[pos] = np.frombuffer(b"RYKMSWBDHV.", np.uint8)[rng.integers(0, 11, len(pos))]
    else:
        a[a == ord("T")] = ord("U")
    return a


def fredge_reads(per, seed, lengths=FREDGE_LENGTHS, paired=False):
    """`per` reads of every class at every length, in a seeded random order (VtReads):
      in_<c>     exact reads inside construct c
      id_<c>     the same with one 1-3 base indel
      sj_<c>     spliced, GT...AG, intron 60..20000: one exon inside c, the other in unique sequence
      ov_first / ov_last / ov_s<k> / ov_e<k>   20 random bases hanging over the genome's start and
                 end and over the start / end of contig k
      hi_last    exact reads that end 60..100 bases before the genome's end: on and past the high
                 border (block end - read length - window length)
      blk1 / blkhigh   exact reads of chr3 starting 0..7 bases in (the second block's first base
                 and low border in the -F -M 1 index) and around FREDGE_BLOCK0_OVER - L - 60 (the
                 first block's high border)
      ch_<kind>  exact reads (half of them inside t150_25, the others in unique sequence of chr2) with
                 N / a lowercase run / IUPAC codes and '.' / U for T
    Every class alternates between the two strands from a random start, the ch_ classes through all
    four combinations of strand and place.
    paired: every read gets a mate -- the reverse complement of an exact read 300..600 bases
    further on (-S fr), as long as the next length of `lengths` (the two ends differ in length when
    `lengths` has more than one) -- and the reverse-strand pairs are swapped, the class's read being
    r2: half the pairs of every class."""
    g, cons = fredge_layout()
    rng = np.random.default_rng(seed)
    f = g.flat
    G = len(f)
    ag_end = np.flatnonzero((f[:-1] == ord("A")) & (f[1:] == ord("G"))).astype(np.int64) + 2
    spans = sorted((c["flat"], c["flat"] + c["length"]) for c in cons.values())
    rows = []

    seen = {}       # class -> [emits so far, a random two bits: the class's first strand and place]

    def turn(cls, step=1):
        """the class's emit counter: its strand alternates from a random start, so every class has
        both strands (and, paired, both orders of the pair) whatever else is emitted between"""
        t = seen.setdefault(cls, [0, int(rng.integers(0, 4))])
        t[0] += step
        return t[0] - step + t[1]

    def emit(src, cls, exact, at):
        src = np.asarray(src, np.uint8)
        st = turn(cls) % 2
        mate = None
        if paired:
            m = min(max(at, 0) + int(rng.integers(300, 601)), G - mate_len)
            mate = revcomp_bytes(f[m:m + mate_len])
        if st:
            rows.append((revcomp_bytes(src), mate, cls, exact, 1) if not paired else (mate, src, cls, exact, 1))
        else:
            rows.append((src, mate, cls, exact, 0))

    def rnd(n):
        return _ACGT[rng.integers(0, 4, n)]

    for li, L in enumerate(lengths):
        mate_len = lengths[(li + 1) % len(lengths)]
        for _ in range(per):
            for name, c in cons.items():
                s = c["flat"] + int(rng.integers(0, c["length"] - L - 3)) if c["length"] > L + 3 else c["flat"]
                s = min(s, G - L - 3)
                emit(f[s:s + L], "in_" + name, True, s)
                emit(_fr_indel(rng, f[s:s + L + 3], L), "id_" + name, False, s)
            for name, c in cons.items():
                if name == "edge_last":
                    continue
                seg = f[c["flat"]:c["flat"] + c["length"]]
                gt = c["flat"] + np.flatnonzero((seg[:-1] == ord("G")) & (seg[1:] == ord("T")))
                cend = int(g.starts[c["contig"]]) + int(g.lens[c["contig"]])
                while True:
                    a = int(rng.integers(30, L - 29))
                    x = int(gt[rng.integers(0, len(gt))])
                    if x - a < c["flat"]:
                        continue
                    d = int(np.exp(rng.uniform(np.log(60), np.log(20000))))
                    k = int(np.searchsorted(ag_end, max(x + d, c["flat"] + c["length"] + 60)))
                    if k >= len(ag_end):
                        continue
                    y = int(ag_end[k])
                    if y - x - 2 > 20000 or y + (L - a) > cend or any(s0 < y + (L - a) and y < e0 for s0, e0 in spans):
                        continue
                    emit(np.concatenate([f[x - a:x], f[y:y + L - a]]), "sj_" + name, False, x - a)
                    break
            emit(np.concatenate([rnd(20), f[:L - 20]]), "ov_first", False, 0)
            emit(np.concatenate([f[G - (L - 20):], rnd(20)]), "ov_last", False, G - L)
            for k in (1, 2):
                s0 = int(g.starts[k])
                emit(np.concatenate([rnd(20), f[s0:s0 + L - 20]]), "ov_s%d" % (k + 1), False, s0)
                emit(np.concatenate([f[s0 - (L - 20):s0], rnd(20)]), "ov_e%d" % k, False, s0 - L)
            s = G - L - int(rng.integers(60, 101))
            emit(f[s:s + L], "hi_last", True, s)
            s = int(g.starts[2]) + int(rng.integers(0, 8))
            emit(f[s:s + L], "blk1", True, s)
            s = int(g.starts[2]) + max(0, FREDGE_BLOCK0_OVER - L - 60 + int(rng.integers(-30, 31)))
            emit(f[s:s + L], "blkhigh", True, s)
            for kind in FREDGE_CHARS:
                c = cons["t150_25"]
                if (turn("ch_" + kind, 0) >> 1) & 1:    # the place changes every second emit, the strand every one
                    s = c["flat"] + int(rng.integers(0, max(1, c["length"] - L)))
                else:
                    s = int(g.starts[1]) + 60000 + int(rng.integers(0, 20000))
                emit(_fr_chars(rng, f[s:s + L], kind), "ch_" + kind, False, s)
    return _vt_finish(rng, rows, paired)


def fredge_retry_reads(n=640, seed=99):
    """161-base reads of the exactly-24-copy array with one small indel each: 6 windows per read
    with up to 24 tied top slots, all of them reported -- more reported slots than
    svg_fragile_batch's first slot buffer (2 * windows + 1024) holds, so its retry runs"""
    g, cons = fredge_layout()
    rng = np.random.default_rng(seed)
    c = cons["t150_24"]
    out = []
    for i in range(n):
        s = c["flat"] + int(rng.integers(0, c["length"] - 165))
        r = _fr_indel(rng, g.flat[s:s + 164], 161)
        out.append(revcomp_bytes(r).tobytes() if i % 2 else r.tobytes())
    return ReadBatch.from_list(out)


CUSTOM_GENOMES = {"lrrow54": lrrow54_genome, "vtedge": vtedge_genome, "fredge": fredge_genome}


def synth_genome(gname):
    if gname in CUSTOM_GENOMES:
        return CUSTOM_GENOMES[gname]()
    from subread_amd.sim import random_genome
    lengths, seed = SYNTH_GENOMES[gname]
    return random_genome(lengths, seed, repeats=(2500, 300, 16, 0.04))


def index_recipe(key):
    """'<genome>_<mode>' -> (genome, gap, memory_mb, force_one_block).  full = -F -B -M 100,
    gapped = the defaults (-M 8000), fullM<n> / gappedM<n> = -F -M <n> / -M <n> (multi-block).
    The genome is chr901, one of SYNTH_GENOMES or one of CUSTOM_GENOMES (vtedge_full, vtedge_gapped)."""
    gname, mode = key.rsplit("_", 1)
    if mode == "full":
        return gname, 1, 100, True
    if mode == "gapped":
        return gname, 3, 8000, False
    m = re.fullmatch(r"(full|gapped)M(\d+)", mode)
    if not m:
        raise KeyError(key)
    return gname, 1 if m.group(1) == "full" else 3, int(m.group(2)), False


def is_multi_block_key(key):
    return "M" in key.rsplit("_", 1)[1]


class IndexCache:
    """Builds the fixture indexes with OUR builder and checks them against the
    reference's md5 known answers before anything votes on them."""

    def __init__(self, root):
        self.root = root
        self.built = {}

    def genome_fasta(self, gname):
        if gname == "chr901":
            path = os.path.join(self.root, "chr901.fa")
            if not os.path.exists(path):
                with gzip.open(os.path.join(GOLD, "chr901.fa.gz"), "rb") as f, open(path, "wb") as o:
                    o.write(f.read())
            return path
        if gname in SYNTH_GENOMES or gname in CUSTOM_GENOMES:
            path = os.path.join(self.root, gname + ".fa")
            if not os.path.exists(path):
                synth_genome(gname).write_fasta(path)
            return path
        raise KeyError(gname)

    def get(self, key):
        if key in self.built:
            return self.built[key]
        import subread_amd as sa
        gname, gap, memory_mb, force = index_recipe(key)
        fa = self.genome_fasta(gname)
        pre = os.path.join(self.root, key)
        sa.build_index(fa, pre, gap=gap, memory_mb=memory_mb, force_one_block=force)
        want = index_md5()["md5"][key]
        for suf, m in want.items():
            got = md5(pre + suf)
            assert got == m, "index %s%s md5 %s != reference %s" % (key, suf, got, m)
        self.built[key] = pre
        return pre


class Case:
    def __init__(self, name):
        self.name = name
        with open(os.path.join(GOLD, name + ".json")) as f:
            self.meta = json.load(f)
        z = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
        self.r1 = ReadBatch(z["r1_seq"], z["r1_off"], z["r1_len"])
        self.r2 = ReadBatch(z["r2_seq"], z["r2_off"], z["r2_len"]) if "r2_seq" in z else None
        self.expected = z["expected"]
        p = SvgParams()
        for (f, _), v in zip(p._fields_, z["params"]):
            setattr(p, f, int(v))
        self.params = p
        self.ends = 2 if self.r2 is not None else 1

    @property
    def index_key(self):
        return self.meta["index"]


def pack_records(out, jout, bm):
    n = out.shape[0]
    parts = [out.view(np.uint8).reshape(n, -1)]
    if jout is not None:
        parts.append(jout.view(np.uint8).reshape(n, -1))
    if bm is not None:
        parts.append(bm.view(np.uint8).reshape(n, -1))
    return np.concatenate(parts, 1)


def describe_mismatch(got, want, ends, mb, limit=5):
    """Human-readable first mismatches: read, end, best, field."""
    bad = np.nonzero((got != want).any(1))[0]
    lines = ["%d of %d reads differ" % (len(bad), got.shape[0])]
    names = MAPPING_DTYPE.names
    for i in bad[:limit]:
        d = np.nonzero(got[i] != want[i])[0]
        msgs = []
        for b in d[:6]:
            if b < ends * mb * 68:
                rec, off = divmod(int(b), 68)
                fld = [n for n in names if MAPPING_DTYPE.fields[n][1] <= off][-1]
                msgs.append("end%d best%d %s" % (rec // mb, rec % mb, fld))
            else:
                msgs.append("byte %d" % b)
        g = got[i, :ends * mb * 68].copy().view(MAPPING_DTYPE)
        w = want[i, :ends * mb * 68].copy().view(MAPPING_DTYPE)
        lines.append("read %d: %s\n  got  %s\n  want %s" % (i, ", ".join(msgs), g, w))
    return "\n".join(lines)
