"""Inputs shared by tests/test_simple_packed_gpu.py and tests/test_simple_packed_host.py: barcode lists as FASTA files,
read batches whose lengths cross the window and tile edges, and constructed windows that pin the end position of rule R1
(csrc/kernels_simple.inc)."""
import random

from qcat_amd import scanner
from qcat_amd.utils import revcomp

# list lengths on both sides of every width class of the simple kernels (csrc/kit.h: simple_width_class)
CLASS_EDGES = (16, 24, 25, 32, 33, 40, 41, 48, 49, 56, 57, 64)
READ_LENGTHS = (0, 1, 15, 23, 24, 25, 149, 150, 151, 400)


def random_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def random_list(seed, n, length):
    """n distinct random barcodes of `length` letters"""
    rng = random.Random(seed)
    seen, out = set(), []
    while len(out) < n:
        s = random_seq(rng, length)
        if s not in seen:
            seen.add(s)
            out.append(s)
    return out


def write_fasta(path, seqs):
    with open(str(path), "w") as fh:
        for i, s in enumerate(seqs):
            fh.write(">bc%04d\n%s\n" % (i + 1, s))
    return str(path)


def detector(tmp_path, seqs, name="list.fa", min_quality=None):
    return scanner.factory(mode="simple", kit=write_fasta(tmp_path / name, seqs), min_quality=min_quality)


def edge_reads(n, seqs, seed):
    """n reads whose lengths cycle through READ_LENGTHS (neighbouring reads -- the two alignments of a lane, the two ends
    of a tile -- differ in length; some windows are shorter than the barcode), most of them holding a noisy barcode copy"""
    rng = random.Random(seed)
    reads = []
    for i in range(n):
        want = READ_LENGTHS[i % len(READ_LENGTHS)]
        bc = seqs[rng.randrange(len(seqs))]
        noisy = "".join(c if rng.random() > 0.08 else rng.choice("ACGT") for c in bc)
        body = random_seq(rng, rng.randrange(0, 40)) + noisy + random_seq(rng, 420)
        if i % 7 == 3:
            body = body[:200] + revcomp(noisy) + body[200:]
        reads.append(body[:want])
    return reads


def _mutate(rng, s, n_mismatch):
    s = list(s)
    for p in rng.sample(range(1, len(s) - 1), n_mismatch):
        s[p] = rng.choice([c for c in "ACGT" if c != s[p]])
    return "".join(s)


def end_windows(bc, seed):
    """{case name: window of up to 150 letters} around barcode `bc`: where the best alignment ends is the point"""
    rng = random.Random(seed)
    m = len(bc)
    w = {}
    w["copy_at_window_end"] = random_seq(rng, 150 - m) + bc                 # row and column maxima meet in H(L, M)
    w["copy_at_offset_0"] = bc + random_seq(rng, 150 - m)
    for k in sorted(set(k for k in (12, 15, 18, 23) if k < m)):
        w["cut_off_after_%d" % k] = random_seq(rng, 150 - k) + bc[:k]       # best in the last row: end_query = L - 1
    w["two_copies"] = random_seq(rng, 20) + bc + random_seq(rng, 30 - min(30, max(0, 2 * m - 100))) + bc
    w["two_copies"] += random_seq(rng, 150 - len(w["two_copies"]))          # the FIRST row that reaches the column maximum
    mid = m // 2
    w["deletion"] = random_seq(rng, 40) + bc[:mid] + bc[mid + 1:] + random_seq(rng, 150 - 40 - m + 1)
    w["insertion"] = random_seq(rng, 40) + bc[:mid] + ("A" if bc[mid] != "A" else "C") + bc[mid:] + random_seq(rng, 150 - 40 - m - 1)
    w["whole_window_is_the_copy"] = bc
    w["copy_then_one_base"] = bc + "A"
    w["window_shorter_than_the_barcode"] = bc[:m - 3]
    # a full-length copy with x mismatches scores m - 2 x in the last COLUMN; a cut-off copy of k = m - 2 x letters at the
    # window's end scores k in the last ROW, at column k < m: a tie of the two borders that QCAT_R1_STRIPED gives to the row
    # (end_query = L - 1) and QCAT_R1_SCALAR to the column (end_query = the degraded copy's last base)
    for x in (1, 2, 3):
        k = m - 2 * x
        filler = 150 - m - k
        if k >= 8 and filler >= 2:
            w["border_tie_%d" % x] = random_seq(rng, filler // 2) + _mutate(rng, bc, x) + random_seq(rng, filler - filler // 2) + bc[:k]
    for name, s in w.items():
        assert len(s) <= 150, (name, len(s))
    return w


def reads_of_windows(windows, seed):
    """reads of 150-letter windows on both ends: window i in front, window i + 1 (reverse-complemented) at the back;
    windows shorter than 150 letters become whole reads"""
    rng = random.Random(seed)
    full = [s for s in windows if len(s) == 150]
    reads = [s for s in windows if len(s) < 150]
    for i, s in enumerate(full):
        reads.append(s + random_seq(rng, 60) + revcomp(full[(i + 1) % len(full)]))
    return reads
