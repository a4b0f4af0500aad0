"""Helpers of the cellCounts voting tests: the golden cases (tests/golden/cellvote/cellvote.npz),
the plain-C model (tests/native/cellvote_model.c, built with the system compiler into a temporary
directory) and the host copy of an index block it runs on."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

import subread_amd as sa
from subread_amd.abi import CELL_HEAD_DTYPE, CELL_SLOT_DTYPE, PackedBatch, ReadBatch
from tests.common import GOLD, ROOT

FIX = os.path.join(GOLD, "cellvote", "cellvote.npz")
INDEXES = ("chr901_full", "chr901_gapped", "synth4242_full", "synth4242_gapped")
SUBREADS = (7, 10, 20)
CASES = [(k, t) for k in INDEXES for t in SUBREADS]

_state = {}


def golden():
    if "z" not in _state:
        _state["z"] = np.load(FIX, allow_pickle=False)
    return _state["z"]


def golden_case(key, total):
    """-> (PackedBatch, heads, slots, max_run) of one golden case."""
    z, p = golden(), "%s_n%d_" % (key, total)
    xm = z[p + "xmask"]
    pk = PackedBatch(z[p + "bases"], xm if len(xm) else None, z[p + "starts"], 0, z[p + "lens"])
    return pk, z[p + "heads"].view(CELL_HEAD_DTYPE), z[p + "slots"].view(CELL_SLOT_DTYPE), z[p + "max_run"]


def unpack_ascii(pk):
    """The ASCII reads of a PackedBatch: A/G/C/T by code, N at every exception base."""
    n = len(pk)
    lens = pk.lens.astype(np.int64)
    starts = pk.starts.astype(np.int64) if pk.starts is not None else np.arange(n, dtype=np.int64) * pk.stride
    offs = np.zeros(n, np.uint64)
    if n > 1:
        offs[1:] = np.cumsum(lens[:-1]).astype(np.uint64)
    at = np.repeat(starts - offs.astype(np.int64), lens) + np.arange(int(lens.sum()), dtype=np.int64)
    code = (pk.bases[at >> 4] >> (30 - 2 * (at & 15)).astype(np.uint32)) & 3
    seq = np.frombuffer(b"AGCT", np.uint8)[code]
    if pk.xmask is not None:
        seq = np.where((pk.xmask[at >> 5] >> (31 - (at & 31)).astype(np.uint32)) & 1, np.uint8(ord("N")), seq)
    return ReadBatch(seq, offs, pk.lens)


class _HostIndex(ctypes.Structure):   # svg_host_index, subread_amd/csrc/svg_internal.h
    _fields_ = [("nb", ctypes.c_uint32), ("items", ctypes.c_uint64), ("gap", ctypes.c_int32), ("padding", ctypes.c_int32),
                ("bstart", ctypes.c_void_p), ("keys", ctypes.c_void_p), ("vals", ctypes.c_void_p),
                ("start_point", ctypes.c_uint32), ("length", ctypes.c_uint32), ("start_base_offset", ctypes.c_uint32),
                ("values_bytes", ctypes.c_uint32), ("values", ctypes.c_void_p), ("n_chr", ctypes.c_uint32),
                ("chr_end", ctypes.c_void_p), ("chr_name", ctypes.c_void_p), ("map", ctypes.c_void_p),
                ("map_len", ctypes.c_size_t)]


def host_index(prefix):
    """Block 00 of an index on disk as the arrays the model takes (the library's host loader)."""
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
                    vals=np.ctypeslib.as_array((ctypes.c_uint32 * n).from_address(ix.vals)).copy())
    finally:
        L.svg_host_index_free(ctypes.byref(ix))


def model_lib():
    if "model" not in _state:
        d = tempfile.mkdtemp(prefix="cellvote_model")
        so = os.path.join(d, "cellvote_model.so")
        r = subprocess.run(["gcc", "-std=gnu11", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-pthread", "-o", so,
                            os.path.join(ROOT, "tests", "native", "cellvote_model.c")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        L = ctypes.CDLL(so)
        vp = ctypes.c_void_p
        L.cellvote_model.restype = ctypes.c_int64
        L.cellvote_model.argtypes = [ctypes.c_uint32, ctypes.c_int, vp, vp, vp, vp, vp, vp, ctypes.c_uint64, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_int, vp, vp]
        _state["model"] = L
    return _state["model"]


def model_vote(index, batch, total_subreads=10, max_indel_length=5, threads=16):
    """The model over `index` (host_index() or VoteIndex.export()) for an ASCII ReadBatch ->
    (heads, slots), or None where svg_cell_vote_batch refuses the arguments."""
    n = len(batch)
    heads = np.zeros(n, CELL_HEAD_DTYPE)
    slots = np.zeros(max(1, n * 51), CELL_SLOT_DTYPE)
    k = model_lib().cellvote_model(index["buckets"], index["gap"], index["bstart"].ctypes.data, index["keys"].ctypes.data,
                                   index["vals"].ctypes.data, batch.seq.ctypes.data, batch.offsets.ctypes.data,
                                   batch.lens.ctypes.data, n, int(total_subreads), int(max_indel_length), int(threads),
                                   heads.ctypes.data, slots.ctypes.data)
    if k < 0:
        return None
    return heads, slots[:k].copy()


def model_vote_sliced(index, batch, total_subreads=10, per=1 << 16, threads=16):
    """model_vote in slices of `per` reads (its staging holds 51 records per read), the heads'
    first_slot counted from the batch's start as svg_cell_vote_batch counts it."""
    hs, ss, at = [], [], 0
    for o in range(0, len(batch), per):
        h, s = model_vote(index, batch.slice(o, min(len(batch), o + per)), total_subreads, threads=threads)
        h["first_slot"][h["applied_subreads"] > 0] += at     # (a skipped read keeps its zero head)
        at += len(s)
        hs.append(h)
        ss.append(s)
    return np.concatenate(hs), np.concatenate(ss)


def index_runs(index):
    """(key, length) of every equal-key run (hit list) of an index block (host_index arrays)"""
    nb, bs = index["buckets"], index["bstart"].astype(np.int64)
    n = int(bs[-1])
    full = (index["keys"][:n].astype(np.int64) & 0xffff) * nb + np.repeat(np.arange(nb, dtype=np.int64), np.diff(bs))
    starts = np.flatnonzero(np.r_[True, full[1:] != full[:-1]])
    return full[starts].astype(np.uint64), np.diff(np.r_[starts, n])


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def slot_rows(heads):
    """Table row of every slot record, from the heads' items."""
    return np.repeat(np.tile(np.arange(17), len(heads)), heads["items"].reshape(-1))


def edge_counts(heads, slots, max_run):
    """Reads of one case that reach each edge of the tally (see tests/test_cellvote_golden.py)."""
    n = len(heads)
    read_of = np.repeat(np.arange(n), heads["n_slots"])
    pos = slots["pos"].astype(np.int64)
    rec = slots["indel_recorder"].astype(np.int64)
    used = np.arange(21)[None, :] < slots["toli"][:, None]
    dist_col = (np.arange(21) % 3 == 2)[None, :] & used
    voter_row = (((pos[:, None] + rec) & 0xffffffff) // 5) % 17
    via = (dist_col & (voter_row != slot_rows(heads)[:, None])).any(1)

    def reads(mask):
        return len(np.unique(read_of[mask]))

    neg = np.bincount(read_of, slots["mask"] != 0, n) > 0
    posi = np.bincount(read_of, slots["mask"] == 0, n) > 0
    return {"row_full": int((heads["items"] == 3).any(1).sum()), "both_masks": int((neg & posi).sum()),
            "toli6": reads(slots["toli"] >= 6), "neighbour_row": reads(via), "run65": int((max_run > 64).sum())}


def long_run_bar(longest):
    """What counts as a long hit list on an index whose longest has `longest` items: more than 64
    where there are such lists, else more than half of the longest there is."""
    return 64 if longest > 64 else longest // 2
