#!/usr/bin/env python3
"""Generate tests/golden/eval_golden.json: what the UNMODIFIED reference tools qcat-eval (`qcat.eval.main`) and qcat-roc
(`qcat.eval_roc.summary`) say about TSV tables this project must evaluate in device memory (qcat_batch_eval).  Dev tool for the
authoring container; see make_golden.py for the stand-ins the reference's imports need (parasail, Bio) -- neither takes part in
an evaluation.

Inputs: the eight stdout tables of the `tsv-auto-batch` and `tsv-dual` runs of cli_golden.json (the reference driver's own
output for the four shipped files), and the tables of the crafted cases of tests/eval_cases.py, formatted with
qcat_amd.cli.tsv_row from their hand-made records.  Per input: the listing and the `-s` line of `qcat-eval --tsv`, and
`summary()` of qcat-roc for q = 0..1000 over the listing read with `pd.read_csv(sep="\\t")` as `create_roc` reads it -- stored as
the rows at which a count changes (`create_roc` itself needs DataFrame.append, which this pandas no longer has: the printed form
of the table is not pinned, its numbers are).  For a case the reference cannot read: the exception's type."""
import contextlib
import io
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402

import eval_cases  # noqa: E402  (tests/ is on the path through make_golden)
from qcat_amd import cli  # noqa: E402

HEADER = "name\tlength\tbarcode\tscore\tkit\tadapter_end\tcomment\n"
ROC_KEYS = ("total", "correct", "incorrect", "true_negative", "false_negative", "false_positive")


def table_of(case, det):
    """the --tsv table of a crafted case: cli.tsv_row over the case's records, as the Python driver prints it"""
    dicts = det._records_to_dicts(eval_cases.records_of(case), det.layouts)
    rows = []
    for title, d in zip(case["titles"], dicts):
        name, comment = cli.split_header(title.rstrip(" \t"))
        rows.append(cli.tsv_row(d, comment, name, "ACGT" * 30) + "\n")
    return HEADER + "".join(rows)


def run_eval(ref_eval, table, summary):
    with tempfile.NamedTemporaryFile("w", suffix=".tsv", delete=False) as fh:
        fh.write(table)
    out = io.StringIO()
    try:
        with contextlib.redirect_stdout(out):
            ref_eval.main(["--tsv", fh.name, "-n", "prog", "-d", "data"] + (["-s"] if summary else []))
    finally:
        os.unlink(fh.name)
    return out.getvalue()


def roc_changes(ref_roc, listing):
    import pandas as pd
    data = pd.read_csv(io.StringIO(listing), sep="\t")
    rows, last = [], None
    for q in range(0, 1001):
        counts = ref_roc.summary(data["truebc"], data["bc"], data["score"], q / 10.0)
        row = [int(counts[k]) for k in ROC_KEYS]
        if row != last:
            rows.append([q] + row)
            last = row
    return rows


def main():
    make_golden.install_standins()
    make_golden.import_reference()
    import qcat.eval as ref_eval
    import qcat.eval_roc as ref_roc

    with open(os.path.join(HERE, "cli_golden.json")) as fh:
        runs = json.load(fh)["runs"]
    inputs = []
    for run in runs:
        if run["variant"]["tag"] in ("tsv-auto-batch", "tsv-dual") and run["file"] in ("nbd103.fastq", "pbk004.fastq", "rab204.fastq", "rbk004.fastq"):
            inputs.append({"name": "%s:%s" % (run["variant"]["tag"], run["file"]), "table": run["stdout"]})
    assert len(inputs) == 8
    scanners = {"epi": eval_cases.epi_scanner(), "dual": eval_cases.dual_scanner()}
    for case in eval_cases.cases():
        inputs.append({"name": "case:" + case["name"], "table": table_of(case, scanners[case["kit"]]), "refused": case.get("refused")})
    out = []
    seen = {"CORRECT": 0, "INCORRECT": 0, "FN": 0, "FP": 0, "TN": 0, "buckets": set()}
    for item in inputs:
        entry = {"name": item["name"], "table": item["table"]}
        if item.get("refused"):
            try:
                run_eval(ref_eval, item["table"], False)
                raise AssertionError("the reference reads " + item["name"])
            except (KeyError, IndexError, TypeError) as e:
                entry["raises"] = type(e).__name__
                entry["refused"] = item["refused"]
            out.append(entry)
            continue
        entry["listing"] = run_eval(ref_eval, item["table"], False)
        entry["summary"] = run_eval(ref_eval, item["table"], True)
        entry["roc"] = roc_changes(ref_roc, entry["listing"])
        if item["name"].startswith("case:"):
            for line in entry["listing"].splitlines()[1:]:
                cols = line.split("\t")
                seen[cols[5]] += 1
                seen["buckets"].add(cols[6])
            seen["TN"] += entry["roc"][0][4]
        out.append(entry)
    assert all(seen[k] >= 5 for k in ("CORRECT", "INCORRECT", "FN", "FP", "TN")) and len(seen["buckets"]) >= 4, seen
    text = json.dumps({"generator": "tests/golden/make_eval_golden.py", "roc_columns": ["q"] + list(ROC_KEYS), "inputs": out}, indent=0, sort_keys=True)
    assert len(text) < 200 * 1024, len(text)
    with open(os.path.join(HERE, "eval_golden.json"), "w") as fh:
        fh.write(text + "\n")
    print("wrote eval_golden.json: %d inputs, %d bytes; crafted cases hold %r" % (len(out), len(text), {k: (v if k != "buckets" else len(v)) for k, v in seen.items()}))


if __name__ == "__main__":
    main()
