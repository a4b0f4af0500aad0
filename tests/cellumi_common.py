"""Shared by the cellCounts UMI-stage tests (tests/test_cellumi_*.py, tests/test_gpu_cellumi.py) and
the fixture maker (tests/golden/cellumi/make_cellumi_golden.py): the plain-C model's loader, the
observation generator of the fixture cases and the class counts read from an entries array."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from subread_amd import abi
from tests.common import ROOT

MODEL_SRC = os.path.join(ROOT, "tests", "native", "cellumi_model.c")
CHECK_SRC = os.path.join(ROOT, "tests", "native", "cellumi_check.c")
ASAN_CMD = ["gcc", "-std=gnu11", "-O1", "-g", "-Wall", "-Wno-unused-function", "-fsanitize=address,undefined",
            "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include")]
FIX = os.path.join(ROOT, "tests", "golden", "cellumi", "cellumi.npz")
FIXTURE_CASES = [(4, 0), (11, 0), (12, 1), (14, 0)]       # (UMI length, with the section of a few thousand entries)
N_SAMPLES = 2
LETTERS = np.frombuffer(b"ACGTN", np.uint8)
_state = {}


def case_name(L):
    return "L%d" % L


def model_lib():
    if "model" not in _state:
        d = tempfile.mkdtemp(prefix="cellumi_model")
        so = os.path.join(d, "cellumi_model.so")
        r = subprocess.run(["gcc", "-std=gnu11", "-O2", "-Wall", "-Werror", "-Wno-unused-function", "-shared", "-fPIC",
                            "-I" + os.path.join(ROOT, "include"), "-o", so, MODEL_SRC], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        L = ctypes.CDLL(so)
        vp, u64, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
        L.cellumi_model.argtypes = [vp, vp, vp, vp, u64, i32, i32, i32, vp, vp, vp, vp, vp, vp]
        L.cellumi_model.restype = i32
        L.cellumi_code.argtypes = [ctypes.c_char_p, i32]
        L.cellumi_code.restype = u64
        L.cellumi_code_hamming.argtypes = [u64, u64]
        L.cellumi_code_hamming.restype = i32
        L.cellumi_half_mask.argtypes = [i32, i32]
        L.cellumi_half_mask.restype = u64
        L.cellumi_packed_code.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
        L.cellumi_packed_code.restype = ctypes.c_uint32
        L.cellumi_decode.argtypes = [u64, i32, ctypes.c_char_p]
        L.cellumi_decode.restype = None
        L.cellumi_hamming_max2.argtypes = [ctypes.c_char_p, ctypes.c_char_p, i32]
        L.cellumi_hamming_max2.restype = i32
        _state["model"] = L
    return _state["model"]


def model_run(sample, cell, gene, umi, L, n_samples=N_SAMPLES, rule=0):
    """The model over observations -> the dict CellCounter.finish(want_entries=True) returns."""
    s = np.ascontiguousarray(sample, np.int32)
    c = np.ascontiguousarray(cell, np.int32)
    g = np.ascontiguousarray(gene, np.int64)
    u = np.ascontiguousarray(umi, np.uint8).reshape(-1)
    n = len(s)
    assert len(c) == n and len(g) == n and u.size == n * L
    ent = np.zeros(n + 1, abi.CELL_UMI_ENTRY_DTYPE)
    cnt = np.zeros(n + 1, abi.CELL_COUNT_DTYPE)
    ne, nc = ctypes.c_uint64(), ctypes.c_uint64()
    rem = np.zeros(n_samples, np.uint64)
    drop = np.zeros(2, np.uint64)
    rc = model_lib().cellumi_model(s.ctypes.data, c.ctypes.data, g.ctypes.data, u.ctypes.data, n, L, n_samples, rule, ent.ctypes.data,
                                   ctypes.byref(ne), cnt.ctypes.data, ctypes.byref(nc), rem.ctypes.data, drop.ctypes.data)
    if rc:
        return rc
    ent, cnt = ent[:ne.value].copy(), cnt[:nc.value].copy()
    firsts = lambda a: np.concatenate([[0], np.cumsum(np.bincount(a["sample"], minlength=n_samples + 1)[1:])]).astype(np.uint64)
    return {"counts": cnt, "count_first": firsts(cnt), "removed_umis": rem, "entries": ent, "entry_first": firsts(ent),
            "dropped_no_sample": int(drop[0]), "dropped_no_cell": int(drop[1])}


def same_result(got, want, entries=True):
    """every byte of entries, counts and removed numbers"""
    assert got["counts"].tobytes() == want["counts"].tobytes()
    assert (got["count_first"] == want["count_first"]).all() and (got["removed_umis"] == want["removed_umis"]).all()
    assert got["dropped_no_sample"] == want["dropped_no_sample"] and got["dropped_no_cell"] == want["dropped_no_cell"]
    if entries:
        assert (got["entry_first"] == want["entry_first"]).all()
        if got["entries"].tobytes() != want["entries"].tobytes():
            bad = np.nonzero(got["entries"] != want["entries"])[0]
            raise AssertionError("entries differ at %s: %s / %s" % (bad[:5], got["entries"][bad[:3]], want["entries"][bad[:3]]))


def _distinct_umis(rng, k, L, alpha, avoid=(), far=()):
    """k distinct random UMIs (uint8 rows) over the first `alpha` letters, none in `avoid`, each at
    distance 2 or more from every row of `far`"""
    out, seen = [], set(bytes(a) for a in avoid)
    while len(out) < k:
        u = LETTERS[rng.integers(0, alpha, L)]
        if bytes(u) in seen or any((u != f).sum() < 2 for f in far):
            continue
        seen.add(bytes(u))
        out.append(u)
    return out


def make_case(L, big, seed):
    """The observations of a fixture case: (sample, cell, gene, umi[n, L]).  Every crafted class gets a
    (cell, gene) of its own (cells from 100 on), the random part uses cells 0..5 and -1, samples 0..2."""
    rng = np.random.default_rng(seed)
    S, C, G, U = [], [], [], []
    half = L // 2

    def put(sample, cell, gene, umi, times=1):
        for _ in range(times):
            S.append(sample), C.append(cell), G.append(gene), U.append(np.asarray(umi, np.uint8))

    cell = [100]

    def new_cell():
        cell[0] += 1
        return cell[0]

    # records with gene lists of 1 and of 3 genes over few cells and short-alphabet UMIs: sections of
    # 1 and 2 entries, merges, equal supports, N, cell -1, sample 0, and step 2 over three genes
    for _ in range(900):
        s, c = int(rng.integers(0, 3)), int(rng.integers(-1, 6))
        u = LETTERS[rng.integers(0, 5 if rng.random() < 0.1 else 3, L)]
        genes = rng.choice(40, 3, replace=False) if rng.random() < 0.3 else [int(rng.integers(0, 40))]
        for g in genes:
            put(s, c, int(g) * 53639, u)
    # lone observations: sections of exactly one entry and (cell, UMI) sections of one
    for k in range(40):
        put(1 + k % 2, new_cell(), 7, _distinct_umis(rng, 1, L, 4)[0])
    # sections of exactly k entries
    for k in (2, 30, 31, 32, 64, 65):
        for j in range(6):
            c = new_cell()
            for u in _distinct_umis(rng, k, L, 5 if L > 4 else 4):
                put(1 + j % 2, c, 11, u, int(rng.integers(1, 4)))
    for j in range(5):
        c = new_cell()
        for u in _distinct_umis(rng, 210 + 10 * j, L, 5):
            put(1 + j % 2, c, 12, u, int(rng.integers(1, 3)))
    if big:
        c = new_cell()
        for u in _distinct_umis(rng, 3000, L, 4):
            put(2, c, 13, u, 1 + (rng.random() < 0.2))
    # chains: B merges into A, C is within 1 of B and 2 from A
    for j in range(6):
        c = new_cell()
        a = _distinct_umis(rng, 1, L, 2)[0]
        p, q = rng.choice(L, 2, replace=False) if L > 1 else (0, 0)
        b = a.copy(); b[p] = LETTERS[2 + (a[p] == LETTERS[2])]
        cc = b.copy(); cc[q] = LETTERS[2 + (a[q] == LETTERS[2])]
        put(1, c, 21, a, 5), put(1, c, 21, b, 3), put(1, c, 21, cc, 2)
    # the order class: E within 1 of X (accepted first, shares E's second half only) and of Y (accepted
    # later, shares E's first half); a second gene holds X's UMI with a support between X's and X's + E's
    for big_section in (0, 1):
        for j in range(6):
            c = new_cell()
            e = LETTERS[rng.integers(0, 2, L)]
            x, y = e.copy(), e.copy()
            x[int(rng.integers(0, half))] = LETTERS[2]
            y[half + int(rng.integers(0, half))] = LETTERS[3]
            put(2, c, 31, x, 9), put(2, c, 31, y, 7), put(2, c, 31, e, 2)
            put(2, c, 32, x, 10)
            if big_section:
                for u in _distinct_umis(rng, 33, L, 5, far=(x, y, e)):
                    put(2, c, 31, u, 1)
    # step 2: equal top supports (removed), a strictly greater one (counted), and survivors that only
    # became unequal through step 1's added support
    for j in range(6):
        u = _distinct_umis(rng, 1, L, 4)[0]
        c = new_cell()
        put(1, c, 41, u, 2), put(1, c, 42, u, 2), put(1, c, 43, u, 1)
        c = new_cell()
        put(1, c, 41, u, 3), put(1, c, 42, u, 2)
        c = new_cell()
        v = u.copy(); v[0] = LETTERS[(np.nonzero(LETTERS == u[0])[0][0] + 1) % 4]
        put(1, c, 41, u, 3), put(1, c, 42, u, 3), put(1, c, 41, v, 1)
    order = rng.permutation(len(S))
    return (np.array(S, np.int32)[order], np.array(C, np.int32)[order], np.array(G, np.int64)[order], np.array(U, np.uint8)[order])


def class_counts(ent, L):
    """The classes of tests/golden/cellumi (ISSUE list) counted in an entries array in step 1's order."""
    half = L // 2
    umi = np.frombuffer(ent["umi"].tobytes(), np.uint8).reshape(len(ent), abi.CELL_MAX_UMI)[:, :L]
    acc = np.frombuffer(ent["acceptor_umi"].tobytes(), np.uint8).reshape(len(ent), abi.CELL_MAX_UMI)[:, :L]
    out = {"size%d" % k: 0 for k in (1, 2, 30, 31, 32, 64, 65)}
    out.update(hundreds=0, thousands=0, chain=0, order_small=0, order_big=0, equal_support=0, with_n=int((umi == ord("N")).any(1).sum()),
               step2_removed=0, step2_counted=0, step2_three=0, step2_by_step1=0)
    key = ent["sample"].astype(np.int64) << 56 | ent["cell"].astype(np.int64) << 32 | ent["gene"]
    starts = np.concatenate([[0], np.nonzero(np.diff(key))[0] + 1, [len(ent)]])
    merged = ent["outcome"] == abi.CELL_UMI_MERGED
    for a, b in zip(starts[:-1], starts[1:]):
        m = b - a
        if "size%d" % m in out:
            out["size%d" % m] += 1
        out["hundreds"] += 200 <= m < 1000
        out["thousands"] += m >= 2500
        if m < 3 or m > 400:
            continue
        accepted = []
        for i in range(a, b):
            if not merged[i]:
                near = [(umi[i] != umi[k]).sum() < 2 for k in range(a, i) if merged[k]]
                out["chain"] += any(near)
                accepted.append(i)
                continue
            if not acc[i].any():        # (the reference's table no longer names this entry's acceptor)
                continue
            d = [(umi[i] != umi[k]).sum() < 2 for k in accepted]
            lst = next((k for k, x in zip(accepted, d) if x), None)
            look = next((k for k, x in zip(accepted, d) if x and (umi[k, :half] == umi[i, :half]).all()), None)
            if look is None:
                look = next((k for k, x in zip(accepted, d) if x and (umi[k, half:2 * half] == umi[i, half:2 * half]).all()), None)
            took = next((k for k in accepted if (umi[k] == acc[i]).all()), None)
            if lst != look:
                out["order_big" if m > 30 else "order_small"] += 1
                assert took == (look if m > 30 else lst), (a, b, i)
            if took is not None and ent["support"][took] == ent["support"][i]:
                out["equal_support"] += 1
    alive = np.nonzero(~merged)[0]
    k2 = [(int(ent["sample"][i]), int(ent["cell"][i]), umi[i].tobytes()) for i in alive]
    groups = {}
    for i, k in zip(alive, k2):
        groups.setdefault(k, []).append(i)
    for g in groups.values():
        if len(g) < 2:
            continue
        g.sort(key=lambda i: (-int(ent["support_merged"][i]), int(ent["gene"][i])))
        out["step2_three"] += len(g) >= 3
        if ent["outcome"][g[0]] == abi.CELL_UMI_REMOVED:
            out["step2_removed"] += 1
        else:
            out["step2_counted"] += 1
            out["step2_by_step1"] += ent["support"][g[0]] <= ent["support_merged"][g[1]]
    return {k: int(v) for k, v in out.items()}


def load_fixture():
    if "fix" not in _state:
        z = np.load(FIX)
        _state["fix"] = {k: z[k] for k in z.files}
    return _state["fix"]


def fixture_case(L):
    """(sample, cell, gene, umi), the reference's result as a finish() dict, and the mask of merged
    entries whose acceptor the reference's table still names"""
    z, q = load_fixture(), case_name(L) + "_"
    obs = (z[q + "sample"].astype(np.int32), z[q + "cell"], z[q + "gene"].astype(np.int64), z[q + "umi"].reshape(-1, L))
    ent = z[q + "entries"].view(abi.CELL_UMI_ENTRY_DTYPE)
    cnt = z[q + "counts"].view(abi.CELL_COUNT_DTYPE)
    firsts = lambda a: np.concatenate([[0], np.cumsum(np.bincount(a["sample"], minlength=N_SAMPLES + 1)[1:])]).astype(np.uint64)
    want = {"counts": cnt, "count_first": firsts(cnt), "removed_umis": z[q + "removed"].astype(np.uint64), "entries": ent,
            "entry_first": firsts(ent), "dropped_no_sample": int((obs[0] <= 0).sum()),
            "dropped_no_cell": int(((obs[0] > 0) & (obs[1] < 0)).sum())}
    return obs, want, z[q + "acceptor_known"].astype(bool)
