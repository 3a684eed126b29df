"""What qcat_batch_partition must give, restated in numpy (never derived from the code under test): the bin of a read from
``desc.id_slots`` the way tests/test_hip_fullsize.py finds count slots, the kept slice by Python slicing, the order by a
stable argsort, the bases by concatenation.  Plus the read set of the edge test."""
import numpy as np

from qcat_amd import native

EDGE_LENGTHS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 700, 4097]
EDGE_LONG = 100003


def bins_of(desc, layouts, recs):
    """barcode bucket of the count vector per record: slot of the barcode's id (dual: slot1 * n + slot2) for a call with an
    adapter (simple mode: any call), else `none`"""
    nb = len(desc.slot_ids)
    dual, simple = desc.mode == "dual", desc.mode == "simple"
    none = nb * nb if dual else nb
    bins = np.full(len(recs), none, dtype=np.int64)
    has = (recs["barcode_idx"] >= 0) & ((recs["adapter_idx"] >= 0) | simple)
    for t, lay in enumerate(layouts):
        m = has & (recs["adapter_idx"] == (-1 if simple else t))
        s1 = np.array([desc.id_slots[b.id] for b in (lay.barcode_set_1 or [])] or [0])
        if dual:
            s2 = np.array([desc.id_slots[b.id] for b in (lay.barcode_set_2 or [])] or [0])
            bins[m] = s1[recs["barcode_idx"][m]] * nb + s2[recs["barcode2_idx"][m]]
        else:
            bins[m] = s1[recs["barcode_idx"][m]]
    return bins, none


def expected(desc, layouts, reads, recs):
    """reads: list of bytes.  Returns dict(bases=bytes, offsets=uint64[n + 1], bin_first=uint64[bins + 1], source=uint32[n],
    bins=int64[n] (bin per input read))."""
    n = len(reads)
    bins, none = bins_of(desc, layouts, recs)
    n_bins = none + 2
    trimming = bool(desc.desc.trim_reads) and desc.ends == native.ENDS_BOTH
    mrl = int(desc.desc.min_read_length)
    t5, t3 = recs["trim5p"].tolist(), recs["trim3p"].tolist()
    kept = []
    for i, r in enumerate(reads):
        sl = r[t5[i]:t3[i]] if trimming else r                       # the writers' slice
        if mrl > 0 and len(sl) < mrl:
            bins[i] = n_bins - 1                                     # skipped, and nothing else
        kept.append(sl)
    source = np.argsort(bins, kind="stable")
    out = [kept[i] for i in source.tolist()]
    offsets = np.zeros(n + 1, dtype=np.uint64)
    if n:
        np.cumsum(np.array([len(s) for s in out], dtype=np.uint64), out=offsets[1:])
    bin_first = np.searchsorted(bins[source], np.arange(n_bins + 1), side="left").astype(np.uint64)
    return {"bases": b"".join(out), "offsets": offsets, "bin_first": bin_first, "source": source.astype(np.uint32), "bins": bins}


def edge_reads(seed=20261019):
    """about 300 reads over EDGE_LENGTHS, one of EDGE_LONG, the rest near 700: list of bytes"""
    rng = np.random.RandomState(seed)
    lens = []
    for k in range(14):
        lens += EDGE_LENGTHS
    lens = [(n + (k % 7) if n >= 700 and k >= len(EDGE_LENGTHS) else n) for k, n in enumerate(lens)]
    lens.insert(150, EDGE_LONG)
    lens += [690 + 3 * k for k in range(20)]
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    return [letters[rng.randint(0, 4, size=n)].tobytes() for n in lens]


def edge_records(desc, layouts, reads, min_read_length=500):
    """hand-made records for edge_reads: bins cycle over a few barcodes of both templates (most bins stay empty) and `none`;
    trims cycle over (0, len), (5, len - 7), (len, len), (len + 10, 3) and bounds that leave just under min_read_length"""
    recs = np.zeros(len(reads), dtype=native.RESULT_DTYPE)
    n_t = len(layouts)
    for i, r in enumerate(reads):
        n = len(r)
        kind = i % 4
        if kind == 3:                                                # no call
            recs[i]["adapter_idx"], recs[i]["barcode_idx"] = (-1, -1) if i % 8 == 3 else (i % n_t, -1)
        else:
            t = i % n_t
            recs[i]["adapter_idx"] = t
            recs[i]["barcode_idx"] = (0, 5, 17, 95, 40)[(i // 4) % 5] % len(layouts[t].barcode_set_1)
        recs[i]["barcode2_idx"] = -1
        recs[i]["exit_status"] = 0 if recs[i]["barcode_idx"] >= 0 else 1
        trim = i % 6
        if trim == 0:
            t5, t3 = 0, n
        elif trim == 1:
            t5, t3 = 5, max(0, n - 7)
        elif trim == 2:
            t5, t3 = n, n
        elif trim == 3:
            t5, t3 = n + 10, 3
        elif trim == 4:
            t5, t3 = 3, min(n, 3 + min_read_length - 1)              # a read long enough is left one base short
        else:
            t5, t3 = (i * 7) % 23, max(0, n - (i * 5) % 19)
        recs[i]["trim5p"], recs[i]["trim3p"] = t5, t3
    return recs
