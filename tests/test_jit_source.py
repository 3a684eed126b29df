"""The text qcat_amd/jit.py generates for a custom kit is pinned token for token (no library, no GPU needed):
tools/jit_source_digest.py hashes the token stream of jit.generate()'s translation unit -- comments and line layout left
out -- and its attach lists for the custom kits of the suite; tests/golden/jit_source_digests.json holds what the tool gave
before generator and JIT took their struct text from one module (qcat_amd/static_text.py).  A change that moves, shares
or re-lays the text leaves every digest as it is; so does the compiler's input, and the kernels of a custom kit."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("jit_source_digest", os.path.join(ROOT, "tools", "jit_source_digest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_generated_text_of_custom_kits_keeps_its_tokens_and_attach_lists():
    tool = _tool()
    with open(tool.GOLDEN) as fh:
        want = json.load(fh)
    got = tool.digests()
    assert sorted(got) == sorted(want)
    changed = sorted("%s (%s)" % (name, field) for name in want for field in ("source", "attach") if got[name][field] != want[name][field])
    assert not changed, ("jit.generate() gives other tokens (source) or other pair / quad lists (attach) for: %s.  If the kernel text "
                         "of custom kits is MEANT to change, regenerate the fixture with `python tools/jit_source_digest.py --write` "
                         "and say so in the change; a refactor must leave it alone." % ", ".join(changed))
