#!/bin/bash
# parity sweeps on the GPU box: tools/fuzz_tiny.py (the one-wave-per-alignment kernels, every intermediate) and
# tools/fuzz_bitslice.py twice over the same seeds -- the barcode kernels forced for small batches, and the adapter kernels
# forced as well (two-stage / four-stage plans by the batch's tile count), and tools/fuzz_geometry.py (kit geometry: set sizes, lengths,
# repeated barcodes on every kernel family; compiles a few hundred small kits the first time);
# tools/gpu_fuzz.sh [bit-sliced seeds, 120] [tiny seeds, 600]
cd $GRAFT_REPO_ROOT
mkdir -p gpurun_out/fuzz
out=$_                      # (the folder just made)
# every step under a time limit of its own; the first one that does not end with status 0 (a mismatch, a time limit, a fault) ends
# the job: nothing more is started on the card after it
step() {
    name=$1; limit=$2; shift 2
    (timeout -k 10 $limit "$@") > $out/$name.txt 2>&1; rc=$?
    tail -1 $out/$name.txt
    [ $rc -eq 0 ] || { echo "$name: exit status $rc -- nothing more is started"; grep -h "MISMATCH\|Error\|Traceback" $out/$name.txt | head -5; exit $rc; }
}
step tiny 900 python tools/fuzz_tiny.py 0 ${2:-600}
QCAT_HIP_BITSLICE_MIN=2048 step barcode 1300 python tools/fuzz_bitslice.py 0 ${1:-120}
QCAT_HIP_BITSLICE_MIN=2048 QCAT_HIP_ADAPTER_BITSLICE_MIN=1 step adapter_forced 1300 python tools/fuzz_bitslice.py 0 ${1:-120}
# (kit geometry: the first run compiles some three hundred small kits, sixteen at a time -- minutes; afterwards they come from the cache)
step geometry 3000 python tools/fuzz_geometry.py --workers 16
grep -c " ok$" $out/tiny.txt $out/barcode.txt $out/adapter_forced.txt $out/geometry.txt
