"""``python -m qcat_amd.eval``: the reference's ``qcat-eval`` (``qcat/eval.py``) and ``qcat-roc`` (``qcat/eval_roc.py``) over text
that stays in device memory.  Every read's title carries ``truebc=<ids>``; the call is held against it as CORRECT, INCORRECT, FN
or FP.

    python -m qcat_amd.eval reads.fastq              the reference's usage: the calls are the ``barcode=`` of the titles (the
                                                     annotated stream this project writes)
    python -m qcat_amd.eval --scan -k KIT reads.fastq    scans first: worth ``qcat --tsv ... | qcat-eval --tsv -``

``-s`` prints the reference's summary line, without it the per-read listing; ``--roc`` prints the counts at the 1001 score
thresholds instead (tab-separated; the numbers are qcat-roc's ``summary()``).  Classes, counts and table come from the device
(qcat_batch_eval); the listing's text columns are formatted here from the class plane and the TSV table."""
from __future__ import print_function

import sys
from argparse import ArgumentParser, RawDescriptionHelpFormatter

from . import config, native
from .scanner import factory

ROC_HEADER = ("total", "correct", "incorrect", "true_negative", "false_negative", "false_positive", "score", "program", "dataset")


def parse_args(argv):
    parser = ArgumentParser(description="qcat-eval and qcat-roc for text in device memory", formatter_class=RawDescriptionHelpFormatter)
    parser.add_argument(dest="FASTX", nargs="?", default=None, help="FASTQ or FASTA file whose titles carry truebc=<ids> (default: stdin)")
    parser.add_argument("-n", "--name", dest="NAME", default="-")
    parser.add_argument("-d", "--dataset", dest="DATASET", default="-")
    parser.add_argument("-s", "--summary", action="store_true", dest="SUMMARY")
    parser.add_argument("--roc", action="store_true", dest="ROC", help="print the counts at the score thresholds 0.0, 0.1 ... 100.0")
    parser.add_argument("--scan", action="store_true", dest="SCAN", help="demultiplex first instead of reading barcode= from the titles")
    parser.add_argument("-k", "--kit", dest="kit", default="auto")
    parser.add_argument("--dual", action="store_true", dest="DUAL")
    parser.add_argument("--simple", action="store_true", dest="SIMPLE")
    parser.add_argument("--trim", action="store_true", dest="TRIM")
    parser.add_argument("--min-read-length", dest="min_length", type=int, default=100)
    parser.add_argument("--detect-middle", action="store_true", dest="DETECT_MIDDLE")
    parser.add_argument("--filter-barcodes", action="store_true", dest="FILTER_BARCODES")
    parser.add_argument("--device", dest="device", type=int, default=0)
    return parser.parse_args(argv)


def parse_reads_info(comment):
    """``_parse_reads_info`` of qcat/eval.py: the ``key=value`` tokens of a comment; a later token replaces an earlier one"""
    info = {}
    if comment:
        for pair in comment.split(" "):
            cols = pair.split("=")
            if len(cols) == 2:
                info[cols[0]] = cols[1]
    return info


def listing_lines(name, dataset, classes, rows):
    """the lines qcat-eval prints per read, from the class plane and ``(read name, comment, call text, score)`` of every
    evaluated read in read order (a dropped read, class 0, has no entry in ``rows``)"""
    rows = iter(rows)
    for cls in classes.tolist():
        if cls == 0:
            continue
        read_id, comment, bc, score = next(rows)
        yield "\t".join((name, dataset, read_id, parse_reads_info(comment)["truebc"], bc, native.EVAL_CLASSES[cls], str(score)))


def summary_line(name, dataset, counts):
    """the line of ``qcat-eval -s`` (qcat/eval.py:168-178): the same float expressions over the device's counts"""
    total, correct, incorrect, fn, fp = (counts[k] for k in ("total", "correct", "incorrect", "fn", "fp"))
    correct_perc = correct * 100.0 / total
    incorrect_perc = (incorrect + fp) * 100.0 / total
    fn_perc = fn * 100.0 / total
    return "\t".join(str(c) for c in (name, dataset, total, correct, incorrect, fn, fp, correct_perc, incorrect_perc, fn_perc))


def roc_lines(name, dataset, roc):
    yield "\t".join(ROC_HEADER)
    for q, row in enumerate(roc.tolist()):
        yield "\t".join([str(c) for c in row] + [repr(q / 10.0), name, dataset])


def evaluate(text, args, listing):
    """(EvalText, rows for :func:`listing_lines` or None) of the bytes of a FASTQ or FASTA file; ``listing``: the per-read rows
    are wanted -- only then does anything per read come back from the device besides the planes"""
    if not args.SCAN:
        ctx = native.NativeContext(args.device)
        batch = native.ResidentBatch.upload_text(ctx, text)
        try:
            out = ctx.eval_text(None, batch, None, from_comment=True)
            title_off, title_len = batch.text_records()[:2] if listing else (None, None)
        finally:
            batch.destroy()
        if not listing:
            return out, None
        rows = []
        for off, length in zip(title_off.tolist(), title_len.tolist()):
            title = text[off:off + length].decode("latin-1").replace("\t", " ")
            read_id, _blank, comment = title.partition(" ")
            rows.append((read_id, comment, parse_reads_info(comment)["barcode"] or "none", -1))
        return out, rows
    mode = "dual" if args.DUAL else ("simple" if args.SIMPLE else "epi2me")
    det = factory(mode=mode, kit="standard" if mode == "simple" else args.kit, enable_filter_barcodes=args.FILTER_BARCODES,
                  scan_middle_adapter=args.DETECT_MIDDLE, device=args.device)
    cfg = config.get_default_config()
    if not listing:
        return det.eval_fastx_text(text, trim=args.TRIM, min_read_length=args.min_length, qcat_config=cfg), None
    out, table = det.eval_fastx_text(text, trim=args.TRIM, min_read_length=args.min_length, qcat_config=cfg, tsv=True)
    rows = []
    for line in table.decode("latin-1").splitlines()[1:]:
        cols = line.split("\t")
        rows.append((cols[0], cols[6], cols[2], float(cols[3])))
    return out, rows


def main(argv=None):
    args = parse_args(sys.argv[1:] if argv is None else argv)
    if args.FASTX:
        with open(args.FASTX, "rb") as fh:
            text = fh.read()
    else:
        text = sys.stdin.buffer.read()
    out, rows = evaluate(text, args, listing=not (args.ROC or args.SUMMARY))
    if args.ROC:
        for line in roc_lines(args.NAME, args.DATASET, out.roc):
            print(line)
        return
    if not args.SUMMARY:
        print("program", "dataset", "read_id", "truebc", "bc", "result", "score", sep="\t")
        for line in listing_lines(args.NAME, args.DATASET, out.classes, rows):
            print(line)
    if out.counts["total"] == 0:
        print("No reads found", file=sys.stderr)
        sys.exit(1)
    if args.SUMMARY:
        print(summary_line(args.NAME, args.DATASET, out.counts))


if __name__ == "__main__":
    main()
