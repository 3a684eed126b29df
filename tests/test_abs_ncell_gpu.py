"""The narrow N cell of the bit-sliced ADAPTER kernels on the GPU, at the edges of a template (csrc/abs_core.h: two planes
of row state per N column; the plans come from qcat_amd/abs_plan.py through hipRTC).  A custom kit whose first template
has the shortest leading flank the kit loader accepts before its N run and whose second has the shortest trailing flank:
both are ZERO columns (layout.py takes the first run of N wherever it lies, kit_prepare.inc asks only that the run ends
inside the template), so the N run is the first column of one plan -- its cells read the boundary difference -- and the
border column of the other.  4200 reads and a few degenerate ones, both ends: full tiles of 2048 read ends and a partial
one, the path forced, both pipeline forms (45 columns: a two-stage and a four-stage plan each), against the oracle: per-template raw score and end position, rows, records, counts."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import custom_kits
import oracle_lib
import synth
from qcat_amd import jit, native, scanner

needs_hipcc = pytest.mark.skipif(jit.compiler() is None, reason="neither libhiprtc nor hipcc available")

LEAD0 = "N" * 24 + "TTAACCTTTCTGTTGGTGCTG"                   # no leading flank: the N run starts in column 1
TRAIL0 = "GGTGCTGAAGAAAGTTGTCGG" + "N" * 24                   # no trailing flank: the N run holds the last column


def _kit(folder):
    rng = random.Random(4242)
    bcs = custom_kits.random_barcodes(rng, 12)
    custom_kits.write_kit(folder, "E_5p", "EDGEKIT", LEAD0, bcs)
    custom_kits.write_kit(folder, "E_3p", "EDGEKIT", TRAIL0, bcs)
    return scanner.factory(mode="epi2me", kit="EDGEKIT", kit_folder=folder)


@needs_hipcc
def test_edge_templates_get_two_plane_plans(tmp_path):
    det = _kit(str(tmp_path))
    seqs = sorted(l.sequence for l in det.layouts)
    assert seqs == sorted([LEAD0, TRAIL0])
    src = jit.generate(det.descriptor())[0]
    assert "abs_cell_n2(" in src and "abs_cell_n(" not in src and "static constexpr unsigned char N0[" in src
    info = native.NativeKit(det.descriptor(), jit=True).describe()
    assert info["bitslice_templates"] == 2 + 0x200                 # both templates: a two-stage and a four-stage plan


@pytest.mark.gpu
@needs_hipcc
def test_n_run_at_either_end_of_a_template_matches_the_oracle(tmp_path, monkeypatch):
    det = _kit(str(tmp_path))
    reads = synth.synth_batch(4200, 1018, det.layouts, 0, 1, error_rate=0.08)
    for i in range(0, len(reads), 11):                                # windows off the path: short reads, an N in the window
        reads[i] = reads[i][:30 + (i % 200)] if i % 2 else reads[i][:50] + "N" + reads[i][51:]
    reads += ["", "ACGTN" * 40, ("ACG" * 80)[:170], "A" * 300, "AC" * 160]
    d = det.descriptor()
    o_recs, o_cnt, o_traces, o_rows = oracle_lib.scan(d, reads, counts=True, trace=True, rows=True, threads=8)
    kit_h = native.NativeKit(d, jit=True)
    assert kit_h.describe()["bitslice_templates"] == 2 + 0x200
    bases, offsets = native.pack_reads(reads)
    assert 2 * 2048 < len(reads) < 3 * 2048                           # per template: two full tiles' worth of reads and a partial one
    monkeypatch.setenv("QCAT_HIP_ADAPTER_BITSLICE_MIN", "1")
    for stages in ("2", "4"):
        monkeypatch.setenv("QCAT_HIP_ABS_STAGES", stages)
        ctx = native.NativeContext(0)
        lib = native.HipLibrary.get().lib
        native.HipLibrary.get().check(lib.qcat_ctx_set_timing(ctx.handle, 1))
        cnt = np.zeros(d.n_count_buckets, dtype=np.int64)
        recs, traces, rows = ctx.scan(kit_h, bases, offsets, counts=cnt, trace=True, rows=True)
        names = (C.c_char_p * 16)()
        ms = (C.c_float * 16)()
        ran = [names[i].decode() for i in range(lib.qcat_ctx_last_timing(ctx.handle, names, ms, 16))]
        assert "k_adapter_bitslice" in ran, ran
        for n in ("tpl_raw", "tpl_end"):
            assert np.array_equal(traces[n], o_traces[n]), (stages, n)
        assert recs.tobytes() == o_recs.tobytes() and np.array_equal(rows, o_rows) and np.array_equal(cnt, o_cnt)
