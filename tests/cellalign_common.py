"""Helpers of the svg_cell_align_batch tests: the golden cases
(tests/golden/cellalign/cellalign.npz), the plain-C model (tests/native/cellalign_model.c, built
with the system compiler into a temporary directory) and the host copy of an index block with its
.array image."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

import subread_amd as sa
from subread_amd.abi import CELL_ALN_DTYPE, CELL_ALN_HEAD_DTYPE, PackedBatch, SvgCellAlignParams
from tests.cellvote_common import INDEXES, SUBREADS, _HostIndex
from tests.common import GOLD, ROOT

FIX = os.path.join(GOLD, "cellalign", "cellalign.npz")
DEFAULTS = dict(total_subreads=10, max_indel_length=5, min_votes_per_mapped_read=3,
                max_differential_from_top_vote_number=2, max_mismatching_bases_in_reads=3,
                min_mapped_length_for_mapped_read=40, max_reported_alignments_per_read=1)
# the issue's second parameter set, on one full and one gapped index
SECOND = dict(max_reported_alignments_per_read=5, max_mismatching_bases_in_reads=10, min_votes_per_mapped_read=1)
CASES = [(k, t, "default") for k in INDEXES for t in SUBREADS] + [("synth4242_full", 10, "second"),
                                                                   ("chr901_gapped", 10, "second")]
EXON_TAIL = 512   # SVG_CELL_EXON_TAIL

_state = {}


def case_params(total, which):
    p = dict(DEFAULTS, total_subreads=total)
    if which == "second":
        p.update(SECOND)
    return p


def golden():
    if "z" not in _state:
        _state["z"] = np.load(FIX, allow_pickle=False)
    return _state["z"]


def golden_case(key, total, which):
    """-> (PackedBatch, exon starts, exon stops, heads, alns) of one golden case."""
    z, p = golden(), "%s_n%d_%s_" % (key, total, which)
    xm = z[p + "xmask"]
    pk = PackedBatch(z[p + "bases"], xm if len(xm) else None, z[p + "starts"], 0, z[p + "lens"])
    ex = z[p + "exons"].reshape(-1, 2)
    return (pk, np.ascontiguousarray(ex[:, 0]), np.ascontiguousarray(ex[:, 1]), z[p + "heads"].view(CELL_ALN_HEAD_DTYPE),
            z[p + "alns"].view(CELL_ALN_DTYPE))


def host_index(prefix):
    """Block 00 of an index on disk as the arrays the model takes, the .array image among them."""
    L = sa.lib()
    L.svg_host_index_load.restype = ctypes.c_int
    L.svg_host_index_load.argtypes = [ctypes.c_char_p, ctypes.POINTER(_HostIndex), ctypes.c_int]
    L.svg_host_index_free.argtypes = [ctypes.POINTER(_HostIndex)]
    ix = _HostIndex()
    assert L.svg_host_index_load(str(prefix).encode(), ctypes.byref(ix), 2) == 0, prefix
    try:
        n = max(1, int(ix.items))
        return dict(buckets=int(ix.nb), gap=int(ix.gap),
                    bstart=np.ctypeslib.as_array((ctypes.c_uint32 * (ix.nb + 1)).from_address(ix.bstart)).copy(),
                    keys=np.ctypeslib.as_array((ctypes.c_int16 * n).from_address(ix.keys)).copy(),
                    vals=np.ctypeslib.as_array((ctypes.c_uint32 * n).from_address(ix.vals)).copy(),
                    values=np.ctypeslib.as_array((ctypes.c_uint8 * ix.values_bytes).from_address(ix.values)).copy(),
                    start_base_offset=int(ix.start_base_offset))
    finally:
        L.svg_host_index_free(ctypes.byref(ix))


MODEL_SRC = os.path.join(ROOT, "tests", "native", "cellalign_model.c")


def model_lib():
    if "model" not in _state:
        d = tempfile.mkdtemp(prefix="cellalign_model")
        so = os.path.join(d, "cellalign_model.so")
        r = subprocess.run(["gcc", "-std=gnu11", "-O2", "-Wall", "-Werror", "-Wno-unused-function", "-Wno-format-truncation", "-shared", "-fPIC", "-pthread",
                            "-o", so, MODEL_SRC], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        L = ctypes.CDLL(so)
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        L.cellalign_model.restype = ctypes.c_int64
        L.cellalign_model.argtypes = [u32, ctypes.c_int, vp, vp, vp, vp, u32, u32, vp, u64, vp, vp, vp, u64, vp, vp, vp, vp, vp]
        L.cellalign_model_planes.restype = None
        L.cellalign_model_planes.argtypes = [vp, vp, u64, vp, u64]
        _state["model"] = L
    return _state["model"]


def plane_bits(index):
    bits = index["start_base_offset"] + 4 * len(index["values"]) + EXON_TAIL
    return (min(bits, 1 << 32) + 31) // 32 * 32


def model_align(index, batch, exons=None, want_outside=False, want_edges=False, **params):
    """The model over `index` (host_index()) for an ASCII ReadBatch -> (heads, alns), or None where
    svg_cell_align_batch refuses the parameters.  exons: (starts, stops) or None.  want_outside /
    want_edges: also the per-read counts of bases asked outside the image / the EDGE_* bits."""
    L = model_lib()
    p = SvgCellAlignParams(*[int(dict(DEFAULTS, **params)[k]) for k, _ in SvgCellAlignParams._fields_])
    n = len(batch)
    heads = np.zeros(n, CELL_ALN_HEAD_DTYPE)
    alns = np.zeros(max(1, n * p.max_reported_alignments_per_read), CELL_ALN_DTYPE)
    outside = np.zeros(max(1, n), np.uint32)
    edges = np.zeros(max(1, n), np.uint32)
    planes, bits = None, 0
    if exons is not None and len(exons[0]):
        bits = plane_bits(index)
        planes = np.zeros(bits // 8 * 2, np.uint8)
        a, b = (np.ascontiguousarray(x, dtype=np.uint32) for x in exons)
        L.cellalign_model_planes(a.ctypes.data, b.ctypes.data, len(a), planes.ctypes.data, bits)
    k = L.cellalign_model(index["buckets"], index["gap"], index["bstart"].ctypes.data, index["keys"].ctypes.data,
                          index["vals"].ctypes.data, index["values"].ctypes.data, len(index["values"]),
                          index["start_base_offset"], planes.ctypes.data if planes is not None else None, bits,
                          batch.seq.ctypes.data, batch.offsets.ctypes.data, batch.lens.ctypes.data, n, ctypes.byref(p),
                          heads.ctypes.data, alns.ctypes.data, outside.ctypes.data, edges.ctypes.data)
    if k < 0:
        return None
    if want_edges:
        return heads, alns[:k].copy(), edges[:n]
    if want_outside:
        return heads, alns[:k].copy(), outside[:n]
    return heads, alns[:k].copy()


# cellalign_model.c's EDGE_* bits
EDGES = {"zero_mm": 1, "zero_rlen": 2, "tie": 4, "weight13": 8, "weight_top": 16}


def make_exons(glen, rng):
    """about glen / 1500 exons of 100-400 bases, so that places inside an exon, within 100 bases of one
    and outside both are all common; one exon starts below 100 (no flank bits at all,
    cell-counts.c:953)"""
    n = max(4, glen // 1500)
    starts = np.sort(rng.integers(200, glen - 600, n)).astype(np.uint32)
    stops = (starts + rng.integers(100, 400, n)).astype(np.uint32)
    return np.r_[np.uint32(40), starts], np.r_[np.uint32(180), stops]


CHECK_SRC = os.path.join(ROOT, "tests", "native", "cellalign_check.c")
ASAN_CMD = ["gcc", "-std=gnu11", "-O1", "-g", "-Wall", "-Wno-unused-function", "-Wno-format-truncation",
            "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-pthread"]


def write_case(path, index, batch, exons, params, heads, alns):
    """one case as cellalign_check.c reads it: 16 u64 (sizes and parameters), then the arrays"""
    a, b = (np.ascontiguousarray(x, dtype=np.uint32) for x in exons)
    p = [int(dict(DEFAULTS, **params)[k]) for k, _ in SvgCellAlignParams._fields_]
    seq = np.ascontiguousarray(batch.seq)
    hdr = np.array([index["buckets"], index["gap"], len(index["keys"]), len(index["values"]), index["start_base_offset"],
                    len(a), len(seq), len(batch), len(alns)] + p, np.uint64)
    assert len(hdr) == 16
    with open(path, "wb") as f:
        for x in (hdr, index["bstart"], index["keys"], index["vals"], index["values"], a, b, seq,
                  batch.offsets.astype(np.uint64), batch.lens.astype(np.uint16), raw(heads), raw(alns)):
            f.write(np.ascontiguousarray(x).tobytes())


def asan_check(hosts, d):
    """Builds cellalign_check.c with the sanitizers and runs it on every golden case."""
    from tests.cellvote_common import unpack_ascii
    exe = os.path.join(d, "cellalign_check")
    r = subprocess.run(ASAN_CMD + ["-o", exe, CHECK_SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for key, total, which in CASES:
        pk, ea, eb, heads, alns = golden_case(key, total, which)
        f = os.path.join(d, "case.bin")
        write_case(f, hosts[key], unpack_ascii(pk), (ea, eb), case_params(total, which), heads, alns)
        r = subprocess.run([exe, f], capture_output=True, text=True)
        assert r.returncode == 0, (key, total, which, r.stdout[-2000:], r.stderr[-4000:])


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def cigar_ops(alns):
    """per record: the set of operation letters of its CIGAR"""
    return [set(ch for ch in c.decode() if not ch.isdigit()) for c in alns["cigar"]]
