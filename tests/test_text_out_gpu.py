"""What the text products of a resident batch share on one context (qcat_amd/csrc/text_out_host.inc): the one buffer for a
caller's records under the partition, the demultiplexed text, the TSV rows and the annotated stream in turn, the device tables
kept beside their host copies when the name tables change, grow, come back and a call fails in between, and the read-out after
a failed call.  Every result is held, byte for byte, to the same call made alone on a fresh context."""
import re

import numpy as np
import pytest

import synth
from qcat_amd import native, scanner

pytestmark = pytest.mark.gpu

MIN_LEN = 20


class _Layout(object):
    """a layout's name tables with other Barcode ids: what native.TsvNames reads of an AdapterLayout"""

    class _Id(object):
        def __init__(self, id):
            self.id = id

    def __init__(self, layout, shift):
        self.kit = layout.kit
        self._sets = [[self._Id(int(b.id) + shift) for b in (layout.get_barcode_set(s) or [])] for s in (0, 1)]

    def get_barcode_set(self, s):
        return self._sets[s]


@pytest.fixture(scope="module")
def case():
    """64 PBC096 reads of about 200 bases as FASTQ text on the device, scanned with trimming and a minimum length of 20: a few
    reads are shorter than that, one keeps nothing under the trim.  (scanner, kit, batch, A, B, names X, names Y): A the scan's
    records, B the same with the call of every second read taken away, Y the ids of X plus a million."""
    pbc = scanner.factory(kit="PBC096")
    reads = synth.synth_batch(64, 20261021, pbc.layouts, 1, 0, error_rate=0.05, insert_len=80)
    reads = [r[:70] if i in (5, 23, 41) else r for i, r in enumerate(reads)]
    text = "".join("@r{} ch={}\n{}\n+\n{}\n".format(i, i % 7, r, "".join(chr(0x21 + (i + k) % 90) for k in range(len(r))))
                   for i, r in enumerate(reads)).encode()
    kit = native.NativeKit(pbc.descriptor(trim=True, min_read_length=MIN_LEN))
    ctx = native.NativeContext(0)
    batch = native.ResidentBatch.upload_text(ctx, text)
    a, _counts = ctx.scan_resident(kit, batch)
    kept = a["trim3p"].astype(np.int64) - a["trim5p"]
    assert 150 < np.median([len(r) for r in reads]) < 260
    assert (a["barcode_idx"] >= 0).sum() >= 40 and 3 <= (kept < MIN_LEN).sum() <= 10 and (kept <= 0).sum() >= 1
    b = a.copy()
    for field in ("barcode_idx", "barcode2_idx", "adapter_idx"):
        b[field][1::2] = -1
    assert b.tobytes() != a.tobytes()
    x = pbc._tsv_names()
    y = native.TsvNames([_Layout(l, 1000000) for l in pbc.layouts])
    yield pbc, kit, batch, a, b, x, y
    batch.destroy()


def _partition(ctx, kit, batch, names, records):
    p = ctx.partition(kit, batch, records=records)
    bases, offsets = p.batch.download()
    got = (bases.tobytes(), offsets.tobytes(), p.bin_first.tobytes(), p.source.tobytes())
    p.batch.destroy()
    return got


def _demux(ctx, kit, batch, names, records):
    d = ctx.demux_text(kit, batch, records=records)
    return bytes(d.text), d.bin_first_bytes.tobytes(), d.rec_first.tobytes(), d.source.tobytes()


def _tsv(ctx, kit, batch, names, records):
    t = ctx.tsv_text(kit, batch, names, records=records)
    return t.text, t.row_first.tobytes()


def _annot(ctx, kit, batch, names, records):
    t = ctx.annot_text(kit, batch, names, records=records)
    return t.text, t.rec_first.tobytes()


@pytest.fixture(scope="module")
def alone(case):
    """the result of one call on a context that made no other, computed once per (product, names, records)"""
    _pbc, kit, batch, a, b, x, y = case
    cache = {}

    def get(call, names, records):
        key = (call.__name__, "xy"[names is y], "ab"[records is b])
        if key not in cache:
            cache[key] = call(native.NativeContext(0), kit, batch, names, records)
            assert len(cache[key][0]) > 1000
        return cache[key]
    return get


def test_one_records_buffer_serves_every_call_in_turn(case, alone):
    _pbc, kit, batch, a, b, x, _y = case
    ctx = native.NativeContext(0)
    for call, records in ((_partition, a), (_tsv, b), (_annot, a), (_demux, b), (_tsv, a)):
        assert call(ctx, kit, batch, x, records) == alone(call, x, records), (call.__name__, records is a)
    assert alone(_tsv, x, a) != alone(_tsv, x, b) and alone(_annot, x, a) != alone(_annot, x, b)


def test_device_tables_follow_their_host_copies(case, alone):
    """name tables X, Y with longer ids, X again, a call refused for a missing bc_id, X once more -- and, since an id has a
    slot of a fixed size whatever its length, a kit with more slots in between: its blob is larger, so the device buffers move"""
    _pbc, kit, batch, a, _b, x, y = case
    dual = scanner.factory(mode="dual")
    dkit = native.NativeKit(dual.descriptor(trim=True, min_read_length=MIN_LEN))
    nobody = a.copy()
    for field in ("barcode_idx", "barcode2_idx", "adapter_idx"):
        nobody[field] = -1
    assert alone(_tsv, x, a) != alone(_tsv, y, a) and alone(_annot, x, a) != alone(_annot, y, a)
    assert len(re.findall(rb"\t10000\d\d\t", alone(_tsv, y, a)[0])) >= 40 and len(re.findall(rb" barcode=10000\d\d\n", alone(_annot, y, a)[0])) >= 40
    no_ids = native.TsvNamesStruct(kit_name=x.struct.kit_name, bc_id=None, bc2_id=None)
    for call, entry in ((_tsv, "qcat_batch_tsv_text"), (_annot, "qcat_batch_annot_text")):
        ctx = native.NativeContext(0)
        for names in (x, y, x):
            assert call(ctx, kit, batch, names, a) == alone(call, names, a), (entry, names is x)
        total = native.C.c_uint64()
        rc = getattr(ctx.hip.lib, entry)(ctx.handle, kit.handle, batch.handle, a.ctypes.data, native.C.byref(no_ids), 0, native.C.byref(total))
        assert rc == -1 and b"name tables missing" in ctx.hip.lib.qcat_last_error()
        assert call(ctx, kit, batch, x, a) == alone(call, x, a), entry
        none_rows = call(ctx, dkit, batch, dual._tsv_names(), nobody)
        assert none_rows == call(native.NativeContext(0), dkit, batch, dual._tsv_names(), nobody) and none_rows[0].count(b"none") >= 50
        assert call(ctx, kit, batch, y, a) == alone(call, y, a) and call(ctx, kit, batch, x, a) == alone(call, x, a), entry


def test_read_out_after_a_failed_call(case, alone):
    _pbc, kit, batch, a, _b, x, _y = case
    ctx = native.NativeContext(0)
    lib = ctx.hip.lib
    stream = _annot(ctx, kit, batch, x, a)
    assert _tsv(ctx, kit, batch, x, a) == alone(_tsv, x, a)
    bad = a.copy()
    bad["raw_score"][int(np.flatnonzero((a["barcode_idx"] >= 0) & (a["adapter_idx"] >= 0))[3])] = 4000
    with pytest.raises(RuntimeError, match="error -1.*qcat_batch_tsv_text: a called record's .raw_score, score_den. lies outside the kit's score table"):
        ctx.tsv_text(kit, batch, x, records=bad)
    with pytest.raises(RuntimeError, match="error -1.*qcat_ctx_fetch_tsv_text: no TSV text on this context"):
        ctx.hip.check(lib.qcat_ctx_fetch_tsv_text(ctx.handle, None, 0, None))
    assert not lib.qcat_ctx_tsv_text_devptr(ctx.handle) and lib.qcat_ctx_annot_text_devptr(ctx.handle)
    buf = np.empty(len(stream[0]), dtype=np.uint8)
    first = np.zeros(batch.n_reads + 1, dtype=np.uint64)
    ctx.hip.check(lib.qcat_ctx_fetch_annot_text(ctx.handle, buf.ctypes.data, len(buf), first.ctypes.data))
    assert (buf.tobytes(), first.tobytes()) == stream == alone(_annot, x, a)
    rows, files = _tsv(ctx, kit, batch, x, a), _demux(ctx, kit, batch, x, a)
    assert rows == alone(_tsv, x, a) and files == alone(_demux, x, a)
    for name, size, more in (("qcat_ctx_fetch_demux_text", len(files[0]), (None, 0, None, None)), ("qcat_ctx_fetch_tsv_text", len(rows[0]), (None,)),
                             ("qcat_ctx_fetch_annot_text", len(stream[0]), (None,))):
        buf = np.empty(size, dtype=np.uint8)
        with pytest.raises(RuntimeError, match="error -1.*%s: the buffer is shorter than the text" % name):
            ctx.hip.check(getattr(lib, name)(ctx.handle, buf.ctypes.data, size - 1, *more))
        ctx.hip.check(getattr(lib, name)(ctx.handle, buf.ctypes.data, size, *more))
        assert buf.tobytes() == {"demux": files, "tsv": rows, "annot": stream}[name.split("_")[3]][0]
