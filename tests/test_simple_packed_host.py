"""Simple mode on the packed end-tracking kernels (csrc/kernels_simple.inc), the part that needs no device: which kits
the path takes (qcat_kit_describe().packed), the switch that turns it off, and -- on the CPU oracle alone -- that the
constructed windows of tests/simple_cases.py do what they were built for."""
import numpy as np
import pytest

import helpers
import oracle_lib
import simple_cases
from qcat_amd import native, scanner


@pytest.mark.parametrize("which", ["standard", "extended"])
def test_bundled_lists_take_the_packed_path(which):
    det = scanner.factory(mode="simple", kit=which)
    assert native.NativeKit(det.descriptor()).describe()["packed"] == 1
    assert native.NativeKit(det.descriptor(ends=native.ENDS_5P)).describe()["packed"] == 1


@pytest.mark.parametrize("length", [16, 24, 25, 32, 33, 40, 41, 64])
def test_lists_of_one_length_with_a_width_class_take_the_packed_path(length, tmp_path):
    det = simple_cases.detector(tmp_path, simple_cases.random_list(length, 5, length))
    assert native.NativeKit(det.descriptor()).describe()["packed"] == 1


def test_lists_without_a_class_and_ragged_lists_stay_on_the_general_kernel(tmp_path):
    det = simple_cases.detector(tmp_path, simple_cases.random_list(1, 5, 15), "short.fa")
    assert native.NativeKit(det.descriptor()).describe()["packed"] == 0
    ragged = simple_cases.random_list(2, 3, 24) + simple_cases.random_list(3, 2, 20)
    det = simple_cases.detector(tmp_path, ragged, "ragged.fa")
    assert native.NativeKit(det.descriptor()).describe()["packed"] == 0


def test_the_other_modes_keep_their_answer():
    for mode, kit in (("epi2me", "NBD103/NBD104"), ("epi2me", "PBC096")):
        assert native.NativeKit(scanner.factory(mode=mode, kit=kit).descriptor(), jit=False).describe()["packed"] == 1


def test_the_switch_exists():
    assert "NO_SIMPLE_PACKED" in native.options()
    assert native.get_option("NO_SIMPLE_PACKED") is None
    native.set_option("NO_SIMPLE_PACKED", 1)
    try:
        assert native.get_option("NO_SIMPLE_PACKED") == 1
    finally:
        native.set_option("NO_SIMPLE_PACKED", None)


def test_the_constructed_windows_do_what_they_were_built_for_in_the_oracle(tmp_path):
    """The oracle alone.  (1) The border-tie windows separate QCAT_R1_STRIPED from QCAT_R1_SCALAR in the oracle's alignment
    routine (qo_sg_rule): striped ends the alignment on the window's last base, scalar on the degraded copy's.  (2) The
    oracle's SIMPLE SCAN places a barcode alignment's end in the striped order under either `r1_rule` (qo_scan_simple, as
    k_scan_simple does: the rule moves adapter alignments only), so its traces do not move with the rule -- and on those
    windows a kernel that took the scalar order under `r1_rule = scalar` would be caught by the GPU tests.  (3) The other
    windows end where they were built to end."""
    from qcat_amd import config
    table = config.qcatConfig().matrix_barcode.table
    differing = 0
    for length in simple_cases.CLASS_EDGES:
        seqs = simple_cases.random_list(100 + length, 3, length)
        det = simple_cases.detector(tmp_path, seqs, "l%d.fa" % length)
        windows = simple_cases.end_windows(seqs[1], 7 * length)
        ties = [n for n in windows if n.startswith("border_tie_")]
        assert ties, length
        here, parted = 0, set()
        for n in ties:
            a = oracle_lib.sg(windows[n], seqs[1], 1, 1, table, rule=native.R1_STRIPED)
            b = oracle_lib.sg(windows[n], seqs[1], 1, 1, table, rule=native.R1_SCALAR)
            assert a[0] == b[0]
            if a[1] != b[1]:
                assert a[1] == 149 and b[1] < 149, (length, n, a, b)
                here += 1
                parted.add(n)
        assert here >= 1, length                       # every class edge has a window on which the two orders part
        differing += here
        reads = simple_cases.reads_of_windows(list(windows.values()), length)
        ends = {}
        for rule in ("striped", "scalar"):
            with helpers.r1_rule(rule):
                _, traces = oracle_lib.scan(det.descriptor(), reads, trace=True)
            ends[rule] = traces["best_end"].copy()
        assert np.array_equal(ends["striped"], ends["scalar"])
        names = list(windows)
        full = [n for n in names if len(windows[n]) == 150]
        first_full = sum(1 for n in names if len(windows[n]) < 150)
        longest_cut = "cut_off_after_%d" % max(k for k in (12, 15, 18, 23) if k < length)
        for i, n in enumerate(full):
            e5 = int(ends["striped"][2 * (first_full + i)])
            if n == "copy_at_offset_0":
                assert e5 == length - 1, (length, n, e5)
            if n in (longest_cut, "copy_at_window_end") or n in parted:     # (a shorter cut may lose to a chance alignment)
                assert e5 == 149, (length, n, e5)
            if n == "two_copies":
                assert e5 == 20 + length - 1, (length, n, e5)
    assert differing >= len(simple_cases.CLASS_EDGES)
