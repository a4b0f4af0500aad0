"""CPU checks of what svg_cell_counter_finish stands on: the record layouts against the header, the
3-bit UMI code that ships (subread_amd/csrc/svg_cell_umi.h, which svg_cell_count.hip includes, reached
here through the model's library: its order against memcmp, its Hamming distance against
cellCounts_hamming_max2_fixlen's rule, its half-key masks, its packed-base table and its decoder), the plain-C model (tests/native/cellumi_model.c) against a
brute-force greedy in Python on sections of 29..33 entries, the two rules of step 1 choosing
different acceptors, the model's refusals, and the sanitizer program
(tests/native/cellumi_check.c: model against a brute-force restatement, no Python, no GPU)."""
import ctypes
import os
import re
import subprocess

import numpy as np

from subread_amd import abi
from tests.cellumi_common import ASAN_CMD, CHECK_SRC, LETTERS, model_lib, model_run
from tests.common import ROOT


def test_structs_match_header():
    src = open(os.path.join(ROOT, "include", "subread_vote.h")).read()
    for name, dt, size in (("svg_cell_count", abi.CELL_COUNT_DTYPE, 16), ("svg_cell_umi_entry", abi.CELL_UMI_ENTRY_DTYPE, 52)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for part in re.findall(r"\w+\s+([^;]+);", body) for n in re.findall(r"(\w+)(?:\[\w+\])?\s*(?:,|$)", part)]
        assert names == list(dt.names), name
        assert dt.itemsize == size
    assert [abi.CELL_UMI_ENTRY_DTYPE.fields[k][1] for k in abi.CELL_UMI_ENTRY_DTYPE.names] == [0, 4, 8, 12, 16, 20, 24, 38]
    assert [abi.CELL_COUNT_DTYPE.fields[k][1] for k in abi.CELL_COUNT_DTYPE.names] == [0, 4, 8, 12]
    body = re.search(r"typedef struct svg_cell_counts \{(.*?)\} svg_cell_counts;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for part in re.findall(r"\w+\s+([^;]+);", body) for n in re.findall(r"\*?(\w+)\s*(?:,|$)", part)]
    assert names == [f[0] for f in abi.SvgCellCounts._fields_]
    assert ctypes.sizeof(abi.SvgCellCounts) == 80
    for k, v in (("MAX_UMI", abi.CELL_MAX_UMI), ("MAX_SAMPLES", abi.CELL_MAX_SAMPLES), ("UMI_COUNTED", abi.CELL_UMI_COUNTED),
                 ("UMI_MERGED", abi.CELL_UMI_MERGED), ("UMI_LOST", abi.CELL_UMI_LOST), ("UMI_REMOVED", abi.CELL_UMI_REMOVED)):
        assert int(re.search(r"#define SVG_CELL_%s\s+(\d+)" % k, src).group(1)) == v
    assert abi.CELL_MAX_CELLS == 1 << 24 and "(1 << 24)" in re.search(r"#define SVG_CELL_MAX_CELLS\s+(.*)", src).group(1)


def test_code_order_is_memcmp_and_code_hamming_is_the_references():
    M = model_lib()
    rng = np.random.default_rng(3511)
    for L in range(1, 15):
        a = LETTERS[rng.integers(0, 5, (400, L))]
        b = a.copy()
        for i in range(400):            # near pairs as well as random ones
            if i % 2:
                b[i] = LETTERS[rng.integers(0, 5, L)]
            else:
                for _ in range(i % 4):
                    b[i, rng.integers(0, L)] = LETTERS[rng.integers(0, 5)]
        for x, y in zip(a, b):
            tx, ty = x.tobytes(), y.tobytes()
            cx, cy = M.cellumi_code(tx, L), M.cellumi_code(ty, L)
            assert cx < 1 << (3 * L)
            assert (cx > cy) - (cx < cy) == (tx > ty) - (tx < ty)          # bytes compare as memcmp
            d = int((x != y).sum())
            assert M.cellumi_code_hamming(cx, cy) == d
            assert M.cellumi_hamming_max2(tx, ty, L) == min(d, 2)             # :3511 stops at 2: only "< 2" is ever asked
            half = L // 2
            for second in (0, 1):       # the keys of :3570: characters 0 .. half-1 and half .. 2 half-1
                m = M.cellumi_half_mask(L, second)
                assert ((cx ^ cy) & m == 0) == (tx[second * half:(second + 1) * half] == ty[second * half:(second + 1) * half])
            buf = ctypes.create_string_buffer(L)
            M.cellumi_decode(cx, L, buf)
            assert buf.raw == tx
        assert M.cellumi_code(b"ACGU" * 4, L) == 2 ** 64 - 1 or L < 4
    assert M.cellumi_code(b"acgt", 4) == 2 ** 64 - 1 and M.cellumi_code(b"ACG\0", 4) == 2 ** 64 - 1
    # svg_packed_reads' base2int (A 0, G 1, C 2, T 3) and the exception bit (N) to the code's characters
    assert [M.cellumi_packed_code(b, 0) for b in range(4)] == [M.cellumi_code(ch, 1) for ch in (b"A", b"G", b"C", b"T")]
    assert [M.cellumi_packed_code(b, 1) for b in range(4)] == [M.cellumi_code(b"N", 1)] * 4


def greedy(ent, L):
    """step 1 over an entries array in step 1's order by the rules as the header states them: -> acceptor index or -1"""
    half = L // 2
    umi = np.frombuffer(ent["umi"].tobytes(), np.uint8).reshape(len(ent), abi.CELL_MAX_UMI)[:, :L]
    key = ent["sample"].astype(np.int64) << 56 | ent["cell"].astype(np.int64) << 32 | ent["gene"]
    starts = np.concatenate([[0], np.nonzero(np.diff(key))[0] + 1, [len(ent)]])
    out = np.full(len(ent), -1)
    for a, b in zip(starts[:-1], starts[1:]):
        acc = []
        for i in range(a, b):
            near = [k for k in acc if (umi[k] != umi[i]).sum() < 2]
            if b - a > 30:
                near = [k for k in near if (umi[k, :half] == umi[i, :half]).all()] or \
                       [k for k in near if (umi[k, half:2 * half] == umi[i, half:2 * half]).all()]
            if near:
                out[i] = near[0]
            else:
                acc.append(i)
    return out


def test_model_equals_a_brute_force_greedy_around_the_threshold():
    rng = np.random.default_rng(3555)
    seen = set()
    for L in (4, 7, 12):
        for size in (29, 30, 31, 32, 33):
            for rep in range(6):
                u = np.unique(LETTERS[rng.integers(0, 3, (4 * size, L))], axis=0)
                u = u[rng.permutation(len(u))[:size]]
                if len(u) < size:
                    continue
                times = rng.integers(1, 4, size)
                umi = np.repeat(u, times, axis=0)
                n = len(umi)
                r = model_run(np.ones(n), np.full(n, 3), np.full(n, 9), umi, L, 1)
                e = r["entries"]
                assert len(e) == size
                want = greedy(e, L)
                merged = e["outcome"] == abi.CELL_UMI_MERGED
                assert (merged == (want >= 0)).all(), (L, size)
                assert all(e["acceptor_umi"][i] == e["umi"][want[i]] for i in np.nonzero(merged)[0]), (L, size)
                supp = e["support"].astype(np.int64).copy()
                np.add.at(supp, want[merged], e["support"][merged])
                assert (supp == e["support_merged"]).all()
                seen.add(size)
    assert seen == {29, 30, 31, 32, 33}


def test_the_two_rules_pick_different_acceptors_and_step2_follows():
    L = 8
    e, x, y = b"AACCAACC", b"GACCAACC", b"AACCAATC"       # x shares e's second half, y its first
    obs = [(1, 5, 31, x)] * 9 + [(1, 5, 31, y)] * 7 + [(1, 5, 31, e)] * 2 + [(1, 5, 32, x)] * 10
    s, c, g, u = (np.array([o[k] for o in obs]) for k in range(3)), None, None, None
    s, c, g = s
    u = np.frombuffer(b"".join(o[3] for o in obs), np.uint8).reshape(-1, L)
    res = {}
    for rule in (1, 2):
        r = model_run(s, c, g, u, L, 1, rule=rule)
        ent = {(int(q["gene"]), bytes(q["umi"])): q for q in r["entries"]}
        res[rule] = (bytes(ent[(31, e)]["acceptor_umi"]), [tuple(int(v) for v in k) for k in r["counts"]])
    assert res[1][0] == x and res[2][0] == y
    # list rule: x has 9 + 2 = 11 > 10: gene 31 counts x; looktable rule: x stays at 9 < 10: gene 32 counts it
    assert res[1][1] == [(1, 5, 31, 2)] and res[2][1] == [(1, 5, 31, 1), (1, 5, 32, 1)]
    assert model_run(s, c, g, u, L, 1)["counts"].tobytes() == model_run(s, c, g, u, L, 1, rule=1)["counts"].tobytes()   # 3 entries: the list rule


def test_model_refusals_and_drops():
    one = lambda **k: model_run(np.array([k.get("s", 1)]), np.array([k.get("c", 0)]), np.array([k.get("g", 0)], np.int64),
                                np.frombuffer(k.get("u", b"ACGT"), np.uint8), 4, 2)
    assert one(u=b"ACGU") == -1 and one(u=b"acgt") == -1 and one(s=3) == -1 and one(c=1 << 24) == -1
    assert one(g=-1) == -1 and one(g=1 << 31) == -1
    assert one(u=b"ACGN")["entries"]["umi"][0] == b"ACGN" and len(one(c=(1 << 24) - 1, g=(1 << 31) - 1)["counts"]) == 1
    r = one(s=0)
    assert r["dropped_no_sample"] == 1 and len(r["entries"]) == 0
    r = one(c=-1)
    assert r["dropped_no_cell"] == 1 and len(r["entries"]) == 0


def test_library_refuses_null_arguments():
    import subread_amd as sa
    L = sa.lib()
    out = ctypes.c_void_p()
    assert L.svg_cell_counter_create(None, 12, 1, ctypes.byref(out)) == -1 and not out.value
    assert L.svg_cell_counter_add(None, None, None, None, None, 0) == -1
    assert L.svg_cell_counter_reset(None) == -1 and L.svg_cell_counter_finish(None, 0, None) == -1
    assert L.svg_cell_count_batch(None, None, None, None, None, None, None, None) == -1
    assert L.svg_cell_count_timing(None, None) == -1
    L.svg_cell_counter_free(None)
    L.svg_cell_counts_free(None)


def test_sanitizer_program(tmp_path):
    exe = str(tmp_path / "cellumi_check")
    r = subprocess.run(ASAN_CMD + ["-o", exe, CHECK_SRC, "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for seed in ("1", "3951"):
        r = subprocess.run([exe, seed], capture_output=True, text=True)
        assert r.returncode == 0, (seed, r.stdout[-2000:], r.stderr[-4000:])
