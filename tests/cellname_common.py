"""What the cellname tests share: the sample sheet and the crafted read names of tests/golden/cellname,
the classes counted from the fixture, the plain-C model (tests/native/cellname_model.c) and the
composition of names for the GPU tests."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from tests.common import ROOT

MODEL_SRC = os.path.join(ROOT, "tests", "native", "cellname_model.c")
CHECK_SRC = os.path.join(ROOT, "tests", "native", "cellname_check.c")
ASAN_CMD = ["gcc", "-std=gnu11", "-O1", "-g", "-Wall", "-Wno-unused-function", "-fsanitize=address,undefined",
            "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-pthread"]
FIX = os.path.join(ROOT, "tests", "golden", "cellname", "cellname.npz")
BCL, FASTQ = 0, 1
LANE_ALL = 99999
MODES = {"bcl": (BCL, 16, 12), "fastq": (FASTQ, 16, 10)}         # mode, barcode length, UMI length
# sample_barcode_list in its order: (lane, sample, index); an index longer than 12 is a dual one
ROWS = [(LANE_ALL, 1, b"ACGTACGT"), (LANE_ALL, 2, b"ACGTACGA"), (2, 3, b"TTGGCCAA"), (LANE_ALL, 4, b"TTGGCCAT"),
        (LANE_ALL, 5, b"GATTACAGCTTACAGA"), (LANE_ALL, 6, b"CATGCATGCAGTCAGTCAGT"), (3, 7, b"GGGGGGGGTTTTTTTT"), (3, 8, b"AAAAAAAACC")]
LINES = [1, 2, 0, 3, 0, 4, 5, 6, 0, 7, 8, 0]                    # sheet line i + 1 -> sample number, 0: absent
N_SAMPLES = 8
QUALS = np.frombuffer(b"#-.0125<ACFGHIJK", np.uint8)
ACGT = b"ACGT"
CLASSES = ["single_d0", "single_d1", "single_refuse_d2", "dual_11", "dual_refuse_20", "read_shorter", "read_longer", "n_in_index",
           "first_of_two_wins", "lane_row_before_all_row", "lane_on_no_row", "rglater_skip", "colon_bcl", "colon_fastq", "input_present",
           "input_absent"]
_state = {}


def mutate(text, where, rng):
    t = bytearray(text)
    for k in where:
        t[k] = rng.choice([c for c in ACGT if c != t[k]])
    return bytes(t)


def compose(rno, bcumi, bq, idx, iq, tail, mode):
    """a name as the readers compose it (cell-counts.c:2206-2212 from BCL; with '|' at 12 from FASTQ)"""
    return b"R%011d" % rno + (b":" if mode == BCL else b"|") + bcumi + b"|" + bq + b"|" + idx + b"|" + iq + tail


def make_names(which, seed):
    """the crafted and random names of one mode: every class of CLASSES its mode can hold, 40 times"""
    mode, bl, ul = MODES[which]
    rng = np.random.default_rng(seed)
    names = []

    def rnd(alphabet, n):
        return bytes(np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), n)])

    def add(idx, lane=1, colon=False, tail=None, n_in_bc=False):
        bcumi = rnd(b"ACGTN" if n_in_bc else ACGT, bl + ul)
        bq = bytearray(QUALS[rng.integers(0, len(QUALS), bl + ul)].tobytes())
        if colon:
            bq[int(rng.integers(0, bl + ul))] = ord(":")            # a quality '9' after the increment of :2229
        iq = QUALS[rng.integers(0, len(QUALS), len(idx))].tobytes()
        if tail is None:
            tail = b"|@RgLater@L%03d" % lane
        names.append(compose(len(names), bcumi, bytes(bq), idx, iq, tail, mode))

    single = [r for r in ROWS if len(r[2]) <= 12]
    dual = [r for r in ROWS if len(r[2]) > 12]
    for rep in range(40):
        for lane_r, _, text in single:
            lane = 1 + rep % 2 if lane_r == LANE_ALL else lane_r
            L = len(text)
            add(text, lane)
            add(mutate(text, [rep % L], rng), lane)
            add(mutate(text, [rep % L, (rep + 3) % L], rng), lane)
        for lane_r, _, text in dual:
            lane = 1 + rep % 4 if lane_r == LANE_ALL else lane_r
            L, h = len(text), len(text) // 2
            add(text, lane)
            add(mutate(text, [rep % h, h + rep % h], rng), lane)                 # (1, 1)
            add(mutate(text, [rep % h, (rep + 2) % h], rng), lane)               # (2, 0)
            add(mutate(text, [h + rep % h, h + (rep + 2) % h], rng), lane)       # (0, 2)
            add(text[:L - 2 - 2 * (rep % 3)], lane)                             # shorter: the halves move
            add(text + rnd(ACGT, 1 + rep % 4), lane)                            # longer
        add(b"ACGTAC"[:4 + rep % 3], 1)                                          # shorter than the single rows
        add(b"ACGTACGT" + rnd(ACGT, 1 + rep % 6), 1)
        add(mutate(b"ACGTACGT", [rep % 8], rng).replace(b"T", b"N", 1) if rep % 2 else b"ACGTACGN", 1)
        add(b"GATTACAGCTTACAGA".replace(b"C", b"N", 1), 2)
        add(b"TTGGCCAA", 2), add(b"TTGGCCAA", 1 + 2 * (rep % 2))                 # the lane's row, and the all-lanes row behind it
        add(b"GGGGGGGGTTTTTTTT", 4 + rep % 5), add(b"AAAAAAAACC", 5 + rep % 4)   # lanes on no row
        add(b"ACGTACGT", 2, tail=b"|L%03d" % (1 + rep % 3))                      # no "@RgLater@"
        add(b"ACGTACGT", 2, tail=b"|@RgLater@L%d and more|text" % (rep % 4))
        add(ROWS[rep % len(ROWS)][2], 1 + rep % 3, colon=True)
        add(ROWS[rep % len(ROWS)][2], 1 + rep % 3, colon=True, n_in_bc=True)
        for _ in range(4):
            add(rnd(ACGT, int(rng.integers(4, 24))), int(rng.integers(1, 5)), n_in_bc=True)
    if mode == FASTQ:
        for rep in range(60):
            bcumi = rnd(b"ACGTN", bl + ul)
            bq = QUALS[rng.integers(0, len(QUALS), bl + ul)].tobytes()
            names.append(b"R%011d|" % len(names) + bcumi + b"|" + bq + b"|input#%04d@L%03d" % (rep % 14, 1 + rep % 4))   # :1829
        for rep in range(20):                                                        # four fields and no lane: "Wrong read name" (:1976)
            names.append(compose(len(names), rnd(ACGT, bl + ul), rnd(b"FGH", bl + ul), b"ACGTACGT", b"FFFFFFFF", b"", mode))
    return names


def scan(name, mode):
    """(fields, sample text position, lane text position or -1) by the rules of the header"""
    seps = [i for i in range(1, len(name)) if name[i:i + 1] == b"|" or (mode == BCL and name[i:i + 1] == b":")][:5]
    lane = -1
    if len(seps) == 5:
        lane = seps[4] + 1
        if name[lane:lane + 9] == b"@RgLater@":
            lane += 9
    return len(seps), seps[2] + 1 if len(seps) >= 3 else -1, lane


def index_run(name, at):
    k = at
    while k < len(name) and name[k] in b"ACGTN":
        k += 1
    return name[at:k]


def row_match(read, row_text):
    """the rule of cellCounts_get_sample_id for one row -> (matches, (p1, p2) or distance)"""
    sl = min(len(read), len(row_text))
    mm = [read[k] != row_text[k] for k in range(sl)]
    if len(row_text) > 12:
        p1, p2 = sum(mm[:sl // 2]), sum(mm[sl // 2:])
        return p1 <= 1 and p2 <= 1, (p1, p2)
    return sum(mm) <= 1, sum(mm)


def class_counts(names, mode, lane, sample):
    """the classes of the issue, counted from names and the REFERENCE's lane and sample alone"""
    c = dict.fromkeys(CLASSES, 0)
    sheet_lanes = {r[0] for r in ROWS}
    for nm, ln, sm in zip(names, lane, sample):
        fields, s3, lp = scan(nm, mode)
        colon = b":" in nm[13:].split(b"|")[1]           # inside the barcode's quality text
        if colon:
            c["colon_bcl" if mode == BCL else "colon_fastq"] += fields == 5
        if lp < 0:
            if nm[s3:s3 + 6] == b"input#":
                c["input_present" if sm > 0 else "input_absent"] += 1
            continue
        k = lp + 1
        while k < len(nm) and nm[k:k + 1].isdigit():
            k += 1
        assert ln == int(nm[lp + 1:k] or b"0"), (nm, ln)
        c["rglater_skip"] += nm[lp - 9:lp] == b"@RgLater@"
        if colon and mode == BCL:
            continue                                      # (the sample text is then a piece of the quality text)
        read = index_run(nm, s3)
        elig = [(i, r) for i, r in enumerate(ROWS) if r[0] == LANE_ALL or r[0] == ln]
        hits = [(i, r, row_match(read, r[2])[1]) for i, r in elig if row_match(read, r[2])[0]]
        if hits:
            i, r, d = hits[0]
            assert sm == r[1], (nm, sm, r)
            if len(r[2]) <= 12 and len(read) == len(r[2]):
                c["single_d0" if d == 0 else "single_d1"] += 1
            if len(r[2]) > 12 and d == (1, 1):
                c["dual_11"] += 1
            c["read_shorter"] += len(read) < len(r[2])
            c["read_longer"] += len(read) > len(r[2])
            c["n_in_index"] += b"N" in read[:len(r[2])]
            c["first_of_two_wins"] += len({h[1][1] for h in hits}) > 1
            c["lane_row_before_all_row"] += r[0] != LANE_ALL and any(h[1][0] == LANE_ALL and h[1][1] != r[1] for h in hits[1:])
        else:
            assert sm == -1, (nm, sm)
            c["single_refuse_d2"] += any(len(r[2]) <= 12 and len(read) == len(r[2]) and row_match(read, r[2])[1] == 2 for _, r in elig)
            c["dual_refuse_20"] += any(len(r[2]) > 12 and row_match(read, r[2])[1] == (2, 0) for _, r in elig)
            c["lane_on_no_row"] += ln not in sheet_lanes and any(row_match(read, r[2])[0] for r in ROWS if r[0] != LANE_ALL)
    return c


def row_text_array(rows=ROWS):
    a = np.zeros((len(rows), 33), np.uint8)
    for i, r in enumerate(rows):
        a[i, :len(r[2])] = np.frombuffer(r[2], np.uint8)
    return a


def model_lib():
    if "model" not in _state:
        d = tempfile.mkdtemp(prefix="cellname_model")
        so = os.path.join(d, "cellname_model.so")
        r = subprocess.run(["gcc", "-std=gnu11", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-pthread", "-o", so, MODEL_SRC],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        L = ctypes.CDLL(so)
        vp, u64, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
        L.cellname_parse_batch.argtypes = [vp, vp, vp, u64, i32, i32, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, i32]
        L.cellname_parse_batch.restype = None
        L.cellname_tallies.argtypes = [u64, vp, vp, vp, vp, vp, i32, vp]
        L.cellname_tallies.restype = None
        L.cellname_max1.argtypes = L.cellname_max1_2p.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
        _state["model"] = L
    return _state["model"]


def join_names(names):
    """(text, offsets, lengths) of a list of names, one behind the other"""
    lens = np.array([len(x) for x in names], np.uint16)
    offs = np.zeros(len(names), np.uint64)
    if len(names) > 1:
        offs[1:] = np.cumsum(lens[:-1].astype(np.uint64))
    text = np.frombuffer(b"".join(names), np.uint8) if names else np.zeros(0, np.uint8)
    return text, offs, lens


def model_parse(names, mode, bl, ul, rows=ROWS, lines=LINES, threads=1, joined=None):
    """-> dict: fields, trimmed_len, lane, sample_no, status (int32 each), packed ([n, 6] uint32), bc and umi texts"""
    text, offs, lens = joined if joined is not None else join_names(names)
    n = len(offs)
    rl = np.array([r[0] for r in rows], np.int32)
    rs = np.array([r[1] for r in rows], np.int32)
    rt = row_text_array(rows)
    ln = np.array(lines, np.int32)
    out = np.zeros((max(n, 1), 5), np.int32)
    packed = np.zeros((max(n, 1), 6), np.uint32)
    bc, umi = np.zeros((max(n, 1), bl), np.uint8), np.zeros((max(n, 1), ul), np.uint8)
    tx = np.ascontiguousarray(text) if len(text) else np.zeros(1, np.uint8)
    model_lib().cellname_parse_batch(tx.ctypes.data, offs.ctypes.data, lens.ctypes.data, n, int(mode == BCL), bl, ul, len(rows), rl.ctypes.data,
                                     rs.ctypes.data, rt.ctypes.data, len(ln), ln.ctypes.data, out.ctypes.data, packed.ctypes.data,
                                     bc.ctypes.data, umi.ctypes.data, threads)
    out, packed = out[:n], packed[:n]
    return {"fields": out[:, 0].copy(), "trimmed_len": out[:, 1].copy(), "lane": out[:, 2].copy(), "sample_no": out[:, 3].copy(),
            "status": out[:, 4].copy(), "packed": packed, "bc": bc[:n], "umi": umi[:n]}


def model_tallies(heads, hits, sample, status, S):
    n = len(heads)
    nrec = np.ascontiguousarray(heads["n_records"], np.uint32)
    first = np.minimum(heads["first_record"].astype(np.int64), max(len(hits) - 1, 0))
    fc = np.ascontiguousarray(hits["contig"][first] if len(hits) else np.zeros(n), np.int32)
    fh = np.ascontiguousarray(hits["nhits"][first] if len(hits) else np.zeros(n), np.uint32)
    sm = np.ascontiguousarray(sample, np.int32)
    st = np.ascontiguousarray(status, np.uint32) if status is not None else None
    out = np.zeros(3 * (S + 1), np.uint64)
    model_lib().cellname_tallies(n, nrec.ctypes.data, fc.ctypes.data, fh.ctypes.data, sm.ctypes.data, st.ctypes.data if st is not None else None, S,
                                 out.ctypes.data)
    return out.reshape(3, S + 1)


def load_fixture():
    if "fix" not in _state:
        z = np.load(FIX)
        _state["fix"] = {k: z[k] for k in z.files}
    return _state["fix"]


def fixture_names(which):
    z = load_fixture()
    text, offs = z[which + "_text"].tobytes(), z[which + "_offs"]
    return [text[int(offs[i]):int(offs[i + 1])] for i in range(len(offs) - 1)]
