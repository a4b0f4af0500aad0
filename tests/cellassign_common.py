"""Helpers of the svg_cell_assign_batch tests: the plain-C model (tests/native/cellassign_model.c
with the host builder subread_amd/csrc/svg_cell_annot.c, built with the system compiler into a
temporary directory), seeded annotations and whitelists, and barcode batches."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from subread_amd.abi import CELL_ALN_DTYPE, CELL_ALN_HEAD_DTYPE, CELL_FEATURE_DTYPE, CELL_HIT_DTYPE, PackedBatch, ReadBatch
from tests.common import ROOT

MODEL_SRC = [os.path.join(ROOT, "tests", "native", "cellassign_model.c"), os.path.join(ROOT, "subread_amd", "csrc", "svg_cell_annot.c")]
CHECK_SRC = os.path.join(ROOT, "tests", "native", "cellassign_check.c")
ASAN_CMD = ["gcc", "-std=gnu11", "-O1", "-g", "-Wall", "-Wno-unused-function", "-fsanitize=address,undefined",
            "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include")]
ACGT = np.frombuffer(b"ACGT", np.uint8)
_state = {}


def model_lib():
    if "model" not in _state:
        d = tempfile.mkdtemp(prefix="cellassign_model")
        so = os.path.join(d, "cellassign_model.so")
        r = subprocess.run(["gcc", "-std=gnu11", "-O2", "-Wall", "-Werror", "-Wno-unused-function", "-shared", "-fPIC",
                            "-I" + os.path.join(ROOT, "include"), "-o", so] + MODEL_SRC + ["-lm"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        L = ctypes.CDLL(so)
        vp, u32, u64, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
        L.cellassign_model_features.restype = ctypes.c_int64
        L.cellassign_model_features.argtypes = [vp, u64, i32, i32, vp, u32, i32, vp, u64, vp, vp, u64]
        L.cellassign_model_barcodes.restype = i32
        L.cellassign_model_barcodes.argtypes = [vp, u64, i32, vp, u64, vp]
        _state["model"] = L
    return _state["model"]


def model_assign(features, allow_multi, chr_end, padding, alns, advance=False):
    """-> (hits, genes) of the model for CELL_ALN_DTYPE records"""
    f = np.ascontiguousarray(features, dtype=CELL_FEATURE_DTYPE)
    a = np.ascontiguousarray(alns, dtype=CELL_ALN_DTYPE)
    ce = np.ascontiguousarray(chr_end, dtype=np.uint32)
    hits = np.zeros(len(a), CELL_HIT_DTYPE)
    cap = max(1, len(a)) * 64
    genes = np.zeros(cap, np.int32)
    k = model_lib().cellassign_model_features(f.ctypes.data, len(f), int(allow_multi), int(advance), ce.ctypes.data, len(ce), int(padding),
                                              a.ctypes.data, len(a), hits.ctypes.data, genes.ctypes.data, cap)
    assert k >= 0, k
    return hits, genes[:k].copy()


def _texts(seqs, L):
    buf = np.zeros((max(1, len(seqs)), L + 1), np.uint8)
    for i, s in enumerate(seqs):
        buf[i, :L] = np.frombuffer(s, np.uint8)
    return buf


def model_barcodes(whitelist, reads):
    """-> cell_barcode_no per read barcode (bytes of the whitelist's length)"""
    L = len(whitelist[0])
    w, r = _texts(whitelist, L), _texts(reads, L)
    out = np.zeros(max(1, len(reads)), np.int32)
    assert model_lib().cellassign_model_barcodes(w.ctypes.data, len(whitelist), L, r.ctypes.data, len(reads), out.ctypes.data) == 0
    return out[:len(reads)]


def make_features(chr_end, padding, rng, per_kb=1.0, genes_per=4, border=6):
    """a seeded annotation over the index's contigs: exons of 50-400 bases, about per_kb per 1000
    bases, both strands, genes of genes_per exons in file order, every tenth feature with the start
    of the one before it (ties), some across a 131,072-base bucket border; the last contig, where
    there are several, gets none"""
    ends = np.asarray(chr_end, np.int64)
    lens = np.diff(np.r_[0, ends]) - 2 * padding + 16
    feats = []
    for c, ln in enumerate(lens):
        if c == len(lens) - 1 and len(lens) > 1:
            continue
        n = max(8, int(ln * per_kb / 1000))
        st = rng.integers(1, max(2, ln - 500), n)
        st[10::10] = st[9:n - 1:10][:len(st[10::10])]
        if ln > 140000:
            st[:border] = 131072 - rng.integers(10, 200, border)
        for s in st:
            feats.append((c, int(s), int(s + rng.integers(50, 400)), len(feats) // genes_per, int(rng.integers(0, 2)), (0, 0, 0)))
    order = rng.permutation(len(feats))
    f = np.array([feats[i] for i in order], CELL_FEATURE_DTYPE)
    return f


def make_whitelist(n, L, rng):
    """n distinct barcodes: a third random, the rest one or two substitutions from an earlier one"""
    seen, out = set(), []
    while len(out) < n:
        if out and rng.random() < 0.66:
            b = bytearray(out[int(rng.integers(0, len(out)))])
            for _ in range(int(rng.integers(1, 3))):
                b[int(rng.integers(0, L))] = b"ACGT"[int(rng.integers(0, 4))]
            b = bytes(b)
        else:
            b = ACGT[rng.integers(0, 4, L)].tobytes()
        if b not in seen:
            seen.add(b)
            out.append(b)
    return out


def make_read_barcodes(whitelist, n, rng):
    """read barcodes by class (i % 6): exact, one substitution at an even position, at an odd one, two
    substitutions, an N at an even position, an N at an odd one"""
    L = len(whitelist[0])
    out = []
    for i in range(n):
        b = bytearray(whitelist[int(rng.integers(0, len(whitelist)))])
        cls = i % 6
        even, odd = 2 * int(rng.integers(0, (L + 1) // 2)), 2 * int(rng.integers(0, L // 2)) + 1
        sub = lambda p: b.__setitem__(p, b"ACGT"[(b"ACGT".index(b[p]) + int(rng.integers(1, 4))) % 4])
        if cls == 1:
            sub(even)
        elif cls == 2:
            sub(odd)
        elif cls == 3:
            sub(even), sub(odd)
        elif cls == 4:
            b[even] = ord("N")
        elif cls == 5:
            b[odd] = ord("N")
        out.append(bytes(b))
    return out


def pack_barcodes(seqs):
    return PackedBatch.pack_numpy(ReadBatch.from_list(list(seqs)))


def brute_barcode(whitelist, cbc):
    """the reference's answer by a scan of the whole whitelist: the exact entry, else the first entry
    with cbc's F key, then with its S key, at Hamming distance 1 (an N is a mismatch)"""
    L = len(cbc)
    for j, w in enumerate(whitelist):
        if w == cbc:
            return j
    for which in (0, 1):
        for j, w in enumerate(whitelist):
            if all(w[2 * k + which] == cbc[2 * k + which] for k in range(L // 2)) and sum(x != y for x, y in zip(w, cbc)) == 1:
                return j
    return -1


# the reference fixture (tests/golden/cellassign/cellassign.npz, make_cellassign_golden.py)
FIX = os.path.join(ROOT, "tests", "golden", "cellassign", "cellassign.npz")
FIXTURE_CASES = [(k, t, "default") for k in ("synth4242_full", "chr901_gapped") for t in (7, 10, 20)] + [
    ("synth4242_full", 10, "second"), ("chr901_gapped", 10, "second")]


def fixture_allow(total, which):
    """allow_multi_overlapping_reads of a fixture case"""
    return int(which == "second" or total == 20)


def renumber_genes(f):
    """gene numbers by first appearance in file order, as the reference numbers them (cell-counts.c:1163)"""
    _, first, inv = np.unique(f["gene"], return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int32)
    rank[np.argsort(first)] = np.arange(len(first), dtype=np.int32)
    g = f.copy()
    g["gene"] = rank[inv]
    return g


def make_whitelist_fixture(n, L, rng, pairs=40):
    """make_whitelist, then `pairs` pairs (A, B) around a barcode X outside the list: A = X with one
    substitution at an even position (X's S row), B = X with one at an odd position (X's F row), A
    before B.  -> (whitelist, the X of every pair)"""
    wl = make_whitelist(n, L, rng)
    seen, xs = set(wl), []
    while len(xs) < pairs:
        x = bytearray(ACGT[rng.integers(0, 4, L)].tobytes())
        a, b = bytearray(x), bytearray(x)
        pa, pb = 2 * int(rng.integers(0, L // 2)), 2 * int(rng.integers(0, L // 2)) + 1
        a[pa] = b"ACGT"[(b"ACGT".index(a[pa]) + 1) % 4]
        b[pb] = b"ACGT"[(b"ACGT".index(b[pb]) + 2) % 4]
        if bytes(x) in seen or bytes(a) in seen or bytes(b) in seen:
            continue
        seen.update((bytes(x), bytes(a), bytes(b)))
        wl += [bytes(a), bytes(b)]
        xs.append(bytes(x))
    return wl, xs


def make_read_barcodes_fixture(whitelist, xs, n, rng):
    """read barcodes by class (i % 8): 0 exact, 1 one substitution at an even position, 2 at an odd
    one, 3 an X of make_whitelist_fixture (the F-row entry wins over an S-row entry of lower number),
    4 an N at an even position, 5 an N at an odd one, 6 two substitutions, 7 an N and a substitution"""
    L = len(whitelist[0])
    sub = lambda b, p, k: b.__setitem__(p, b"ACGT"[(b"ACGT".index(b[p]) + k) % 4])
    out = []
    for i in range(n):
        cls = i % 8
        b = bytearray(xs[int(rng.integers(0, len(xs)))] if cls == 3 else whitelist[int(rng.integers(0, len(whitelist)))])
        even, odd = 2 * int(rng.integers(0, L // 2)), 2 * int(rng.integers(0, L // 2)) + 1
        if cls == 1:
            sub(b, even, int(rng.integers(1, 4)))
        elif cls == 2:
            sub(b, odd, int(rng.integers(1, 4)))
        elif cls == 4:
            b[even] = ord("N")
        elif cls == 5:
            b[odd] = ord("N")
        elif cls == 6:
            sub(b, even, 1), sub(b, odd, 2)
        elif cls == 7:
            sub(b, even, 1)
            b[odd] = ord("N")
        out.append(bytes(b))
    return out


def build_tables(features, chr_end, padding):
    """the host builder's tables in the fixture's form (t_* of fixture_case)"""
    L = model_lib()
    f = np.ascontiguousarray(features, dtype=CELL_FEATURE_DTYPE)
    ce = np.ascontiguousarray(chr_end, dtype=np.uint32)
    L.cellassign_model_tables.restype = ctypes.c_int
    L.cellassign_model_tables.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int] + [ctypes.c_void_p] * 10
    n, nc = len(f), len(ce)
    words = int(sum((int(x) + 1500000) // 131072 + 4 for x in np.diff(np.r_[0, ce.astype(np.int64)])))
    t = dict(start=np.zeros(n, np.uint32), stop=np.zeros(n, np.uint32), strand=np.zeros(n, np.uint8), gene=np.zeros(n, np.int32),
             block_end=np.zeros(n, np.uint32), block_min=np.zeros(n, np.uint32), block_max=np.zeros(n, np.uint32),
             contigs=np.zeros(3 * nc, np.uint32), rev=np.zeros(words, np.uint32))
    counts = np.zeros(2, np.uint32)
    assert L.cellassign_model_tables(f.ctypes.data, n, ce.ctypes.data, nc, int(padding), *[t[k].ctypes.data for k in (
        "start", "stop", "strand", "gene", "block_end", "block_min", "block_max", "contigs", "rev")], counts.ctypes.data) == 0
    for k in ("block_end", "block_min", "block_max"):
        t[k] = t[k][:counts[0]]
    t["rev"] = t["rev"][:counts[1]]
    return t


def fixture():
    if "fix" not in _state:
        _state["fix"] = np.load(FIX, allow_pickle=False)
    return _state["fix"]


def fixture_case(key, total, which):
    """-> dict of one fixture case: pk, barcodes and whitelist (lists of bytes), features, chr_end, heads,
    alns, hits, genes, bcno and the reference's tables t_*"""
    z, p = fixture(), "%s_n%d_%s_" % (key, total, which)
    xm = z[p + "xmask"]
    wl = z[p + "whitelist"].tobytes()
    bc = z[p + "barcodes"].tobytes()
    c = dict(pk=PackedBatch(z[p + "bases"], xm if len(xm) else None, z[p + "starts"], 0, z[p + "lens"]),
             whitelist=[wl[i:i + 16] for i in range(0, len(wl), 16)], barcodes=[bc[i:i + 16] for i in range(0, len(bc), 16)],
             features=z[p + "features"].view(CELL_FEATURE_DTYPE), chr_end=z[p + "chr_end"],
             heads=z[p + "heads"].view(CELL_ALN_HEAD_DTYPE), alns=z[p + "alns"].view(CELL_ALN_DTYPE),
             hits=z[p + "hits"].view(CELL_HIT_DTYPE), genes=z[p + "genes"], bcno=z[p + "bcno"])
    for k in ("start", "stop", "strand", "gene", "block_end", "block_min", "block_max", "contigs", "rev"):
        c["t_" + k] = z[p + "t_" + k]
    return c


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)
