#!/usr/bin/env python3
"""Digests of what qcat_amd.jit.generate() returns for a fixed list of custom kits (no library, no GPU needed):

    source   SHA-256 of the token stream of the generated translation unit: `//` comments deleted, then
             re.findall(r"[A-Za-z_0-9]+|\\S", text) joined by one space -- what the compiler sees, not the line layout
    attach   SHA-256 of repr() of the other four return values (template flags, group flags, pair entries, quads):
             what qcat_kit_attach_code_quads is told about the code object

The kits: every entry of geometry_cases.GENERATED and EXTRA with its switches, the three kits of tests/test_jit.py
(CUSTOM, the dual folder, LONGKIT with its wide-stage template), the shipped dual kit with 49 barcodes in set 2 and all 96
barcodes of PBC096 as a custom set (24 quads).  tests/test_jit_source.py compares the result with
tests/golden/jit_source_digests.json: a change of the kernel text that is NOT meant to change the tokens (layout, comments,
where the text is written) leaves every digest as it is.

    python tools/jit_source_digest.py            print the digests as JSON
    python tools/jit_source_digest.py --write    rewrite tests/golden/jit_source_digests.json (an INTENDED change of the text)"""
import hashlib
import json
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import geometry_cases as gc                   # noqa: E402
from qcat_amd import jit, scanner             # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "jit_source_digests.json")


def tokens(text):
    return " ".join(re.findall(r"[A-Za-z_0-9]+|\S", re.sub(r"//[^\n]*", "", text)))


def kits():
    """[(name, descriptor, jit.generate switches)]"""
    import test_jit
    out = [(name, gc.descriptor(make()), sw) for table in (gc.GENERATED, gc.EXTRA) for name, (make, sw) in sorted(table.items())]
    with tempfile.TemporaryDirectory(prefix="qcat_digest_") as tmp:
        test_jit._custom_kits(tmp)
        dual = os.path.join(tmp, "dual")
        out.append(("test_jit CUSTOM", scanner.factory(mode="epi2me", kit="CUSTOM", kit_folder=tmp).descriptor(), ()))
        out.append(("test_jit dual", scanner.factory(mode="dual", kit_folder=dual).descriptor(), ()))
        out.append(("test_jit LONGKIT", scanner.factory(mode="epi2me", kit="LONGKIT", kit_folder=tmp).descriptor(), ()))
    out.append(("dual set2 49", gc.descriptor(gc.dual_subset_layouts(49), mode="dual"), ()))
    out.append(("PBC096 as custom 96", gc.descriptor(gc.subset_layouts(list(range(96)))), ()))
    return out


def digests():
    """{kit name: {"source": ..., "attach": ...}}"""
    out = {}
    outside = 0                                  # sets of >= 48 targets that leave complete pairs outside their quads
    for name, d, switches in kits():
        res = gc.generate(d, switches)
        assert res == gc.generate(d, switches), "jit.generate is not deterministic for " + name
        out[name] = {"source": hashlib.sha256(tokens(res[0]).encode()).hexdigest(),
                     "attach": hashlib.sha256(repr(tuple(res[1:])).encode()).hexdigest()}
        outside += sum(1 for pairs, quads in zip(res[3], res[4]) if quads and any(bb >= 0 for _, _, bb in pairs))
    assert outside, "no kit has a set with quads AND complete pairs outside them"
    assert len(out) == len(gc.GENERATED) + len(gc.EXTRA) + 5
    return out


def main():
    text = json.dumps(digests(), indent=1, sort_keys=True) + "\n"
    if "--write" in sys.argv[1:]:
        with open(GOLDEN, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
