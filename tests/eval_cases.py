"""The crafted cases of the evaluation in device memory (qcat_batch_eval), shared by tests/golden/make_eval_golden.py -- which feeds
them to the reference's own qcat-eval and qcat-roc -- and tests/test_eval_gpu.py: titles with ``truebc=`` in every form the
tokenizer has to tell apart, and hand-made records whose scores lie on bucket edges.

Two kits.  ``epi``: an EPI2ME kit written here (tests/custom_kits.py) with 130 barcodes, ids 1..130 -- the shipped kits stop at
96 and the lists below need the id 123 -- and a target of 5 + 24 + 11 = 40 bases, so score_den is 40 and raw / den gives 0.0,
60.0, 62.5 and 100.0 exactly (no shipped kit has a denominator that does).  ``dual``: the shipped DUAL kit, denominators 41, 42
and 46: 16 / 41 = 39.02.. lies just above a tenth, 25 / 41 = 60.97.. just below one.

A case: ``name``, ``kit`` (``epi`` / ``dual``), ``titles`` (str, as they stand in the FASTQ text), ``calls`` (per read ``None`` or
``(barcode index, second index or -1, raw score, score_den)``), and for a case the reference cannot read ``refused``: the 1-based
number of the first read it fails on."""
import random
import tempfile

import numpy as np

import custom_kits
from qcat_amd import native, scanner

EPI_DEN = 40
_tmp = []


def epi_scanner():
    """the EPI2ME kit of the cases: 130 random 24-nt barcodes behind 5 bases of context and in front of more than 11"""
    d = tempfile.TemporaryDirectory(prefix="qcat_eval_kit_")
    _tmp.append(d)
    rng = random.Random(40)
    custom_kits.write_kit(d.name, "EVAL40", "EVAL40", "GTTAC" + "N" * 24 + "CAGCACCTGGTGCTGTTAACCTACTTGCC", custom_kits.random_barcodes(rng, 130))
    return scanner.factory(mode="epi2me", kit="EVAL40", kit_folder=d.name)


def dual_scanner():
    return scanner.factory(mode="dual")


def long_title(name, last):
    """a comment longer than 4096 bytes in which the key ``truebc`` begins at every position 0..15 of a 16-byte vector once (the
    title is stored behind '@' at the start of a line: only the differences count); the last one states ``last``"""
    title = name
    for k in range(16):
        title += " p="
        while (len(title) + 1) % 16 != k:
            title += "z"
        title += " truebc=%d ch=%d" % (k + 1, k) + " pad=" + "y" * 250
    return title + " truebc=" + last


def _epi_cases():
    c = []                                                                       # (title, call)

    def add(title, bc, raw=30):
        c.append((title, None if bc is None else (bc - 1, -1, raw, EPI_DEN)))
    add("r0 truebc=1", 1, 40)                                                    # the only token; 100.0
    add("r1 truebc=2 ch=3 read=7", 1, 24)                                        # the first; 60.0
    add("r2 ch=3 truebc=12 read=7", 12, 25)                                      # a middle one; 62.5
    add("r3 ch=3 read=7 truebc=5", None)                                         # the last
    add("r4 truebc=1 ch=3 truebc=2", 2, 0)                                       # twice: the last wins; 0.0
    add("r5 truebc=1 ch=3 truebc=2", 1, 1)
    add("r6 truebc=3 truebc=1=2", 3, 39)                                         # two '=': does not count
    add("r7 truebc=4 xtruebc=1", 1, 40)                                          # another key
    add("r8 truebc=9 truebc", 9, 23)                                             # no '='
    add("r9 truebc=", 1, 24)                                                     # an empty value
    add("r10 truebc=", None)
    for i, bc in enumerate((1, 12, 2, 123, None)):                               # lists
        add("l%d truebc=1,12,3" % i, bc, 24 + i)
    add("l5 truebc=12,none", None)                                               # "none" as an element: CORRECT, and no ROC true negative
    for i in range(5):                                                           # truth none, without and with a call
        add("n%d ch=%d truebc=none" % (i, i), None)
        add("p%d truebc=none ch=%d" % (i, i), 5 + i, (0, 1, 24, 25, 40)[i])
    for i in range(5):
        add("f%d read=%d truebc=%d" % (i, i, 100 + i), None)
    add("b0  truebc=7", 7, 24)                                                   # two blanks in a row
    add("b1 ch=1  truebc=7  x=2", 8, 25)
    add("t0\ttruebc=7\tch=2", 7, 26)                                             # tabs
    add("t1 ch=1\ttruebc=7", 123, 27)
    add(long_title("long0", "130"), 130, 24)
    add(long_title("long1", "1,130"), 16, 25)
    return c


def _dual_cases():
    c = []

    def add(title, bc, bc2=-1, raw=30, den=42):
        c.append((title, None if bc is None else (bc - 1, bc2 - 1, raw, den)))
    add("d0 truebc=3/7", 3, 7, 16, 41)                                           # just above 39.0
    add("d1 ch=1 truebc=3/7", 3, 7, 25, 41)                                      # just below 61.0
    add("d2 truebc=3/7 ch=2", 7, 3, 21, 42)                                      # 50.0; the pair the other way round
    add("d3 truebc=3/7,1/2", 1, 2, 46, 46)                                       # 100.0; a list
    add("d4 truebc=3/7,1/2", 3, 7, 0, 46)
    add("d5 truebc=3/7", None)
    add("d6 truebc=none", None)
    add("d7 truebc=none", 3, 7, 23, 46)
    add("d8 truebc=3", 3, 7, 41, 41)                                             # half of the pair
    add("d9 truebc=3/ ch=4", 3, 7, 42, 42)
    add("d10 truebc=1/2 truebc=3/7", 3, 7, 20, 41)
    return c


def cases():
    out = [{"name": "epi", "kit": "epi", "titles": [t for t, _c in _epi_cases()], "calls": [c for _t, c in _epi_cases()]},
           {"name": "dual", "kit": "dual", "titles": [t for t, _c in _dual_cases()], "calls": [c for _t, c in _dual_cases()]}]
    good = [("g0 truebc=1", (0, -1, 24, EPI_DEN)), ("g1 truebc=2", None), ("g2 truebc=3", (2, -1, 40, EPI_DEN)), ("g3 truebc=4", None)]
    for name, at, title in (("no-truebc", 2, "g1 ch=3 truebd=1"), ("no-comment", 3, "g2"), ("empty-name", 2, " truebc=2"),
                            ("empty-name-called", 1, " truebc=1"), ("name-header", 2, "name1 truebc=2"), ("name-header-called", 3, "names truebc=3")):
        rows = list(good)
        rows[at - 1] = (title, rows[at - 1][1])
        out.append({"name": name, "kit": "epi", "titles": [t for t, _c in rows], "calls": [c for _t, c in rows], "refused": at})
    return out


def records_of(case):
    """the case's calls as qcat_result records: adapter 0 for a called read, everything -1 for the others"""
    recs = np.zeros(len(case["calls"]), dtype=native.RESULT_DTYPE)
    for field in ("barcode_idx", "barcode2_idx", "adapter_idx", "adapter_end"):
        recs[field] = -1
    recs["score_den"] = 1
    for i, call in enumerate(case["calls"]):
        if call is not None:
            recs["barcode_idx"][i], recs["barcode2_idx"][i], recs["raw_score"][i], recs["score_den"][i] = call
            recs["adapter_idx"][i] = 0
            recs["adapter_end"][i] = 30 + i
    return recs


def fastq_of(case):
    """the FASTQ text of a case: every read 120 bases, none dropped"""
    return "".join("@%s\n%s\n+\n%s\n" % (t, "ACGT" * 30, "I" * 120) for t in case["titles"]).encode("latin-1")
