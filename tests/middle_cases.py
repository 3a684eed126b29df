"""Reads, expected staircases and the path runner of the interior-scan boundary sweep (tests/test_middle_boundaries_gpu.py).
No tests here.

--detect-middle leaves the library as one bit per read: exit status 997 or not, decided at `middle_min_score` (50.0 in the
product; a field of the kit descriptor that the device and the oracle both honour).  One batch scanned under a LADDER of
thresholds -- every value 100.0 * r / tlen that a raw barcode score r can produce for the kit's target lengths, 0 and one
rung above the top -- turns the bit into a staircase: the number of rungs at which a read still comes back 997 is its
interior barcode score (the larger of the two strands), pinned to the raw unit.  A wrong adapter score, an end one row off,
the wrong template, the wrong one of the region / whole-window paths or a wrongly clipped region all move that score.

Every read is END5 + spacer + INSERTED + spacer + END3: END5 / END3 are error-free read ends of exactly one window, so that
the end scans call the kit (no interior scan without a called adapter); INSERTED is a copy of one of the kit's templates
with a barcode, on either strand, with substitutions in the barcode and, in some cases, in the flanks.  The builder works
in INTERIOR coordinates: m = len(read) - 2 * max_align_length and the row at which the copy ends (on the copy's strand).

The expected side needs the full oracle (1 ms per read and rung) only five times: without 997 (threshold above every
score), with every called read 997 (threshold below every score) and at three rungs that pin the derivation.  The interior
scores themselves come from oracle_lib.scan_sequences on the interior and on its reverse complement."""
import ctypes as C
import random

import numpy as np

import geometry_cases as gc
import oracle_lib
import synth
from qcat_amd import config, native, scanner, utils

PK_ROWS = 152                   # csrc/kernels_packed.inc: rows of the query that k_adapter_middle stages at a time
MID_CLASS_ROWS = 64             # csrc/kernels_middle.inc: interiors of one tile of 128 differ by up to 63 rows
MID_MAX = 16384                 # ... and the longest interior of the packed path
LEAD = 8                        # random letters in front of the 5' adapter / behind the 3' adapter of a constructed read

#: name -> what scanner.factory takes, the templates of the constructed read ends, which case families
KITS = {
    "NBD": dict(mode="epi2me", kit="NBD103/NBD104", t5=1, t3=0, families="all"),
    "PBC096": dict(mode="epi2me", kit="PBC096", t5=1, t3=0, families="reduced"),
    "DUAL": dict(mode="dual", kit=None, t5=1, t3=0, families="reduced"),
    "AUTO": dict(mode="epi2me", kit=None, t5=3, t3=2, families="reduced"),         # kit-auto: twelve templates of seven kits, reads of PBC096
}


def scoring(name):
    """the configurations of the sweep: "default"; "gap1" (a gap cost other than 2 that keeps the binary16 adapter chains:
    (5 + 2 g) * 128 + 288 g <= 2047 holds for g = 1, not for g = 3 -- the tests ask the library); "n100" (max_align_length
    100: the interior's borders move by 50 letters at either end); "ext0" (extracted_barcode_extension 0: the barcode
    region is the barcode alone -- by default eleven letters more on either side absorb an adapter end that is up to three
    rows off (tools/middle_sensitivity.py), without them the barcode score moves with every row)"""
    cfg = config.qcatConfig()
    if name == "gap1":
        cfg.gap_open = cfg.gap_extend = 1
        cfg.update_matrix()
    elif name == "n100":
        cfg.max_align_length = 100
    elif name == "ext0":
        cfg.extracted_barcode_extension = 0
    elif name != "default":
        raise ValueError(name)
    return cfg


# ---- reads -----------------------------------------------------------------------------------------------------------------
class Read(object):
    """one constructed read: `family` (1 .. 6 of the sweep, 0: the decision filler), `label`, interior length `m`, the row
    at which the copy ends on `strand` ("+": the interior, "-": its reverse complement), `clean`: the copy lies whole
    inside the interior and its flanks carry no change, `special`: the interior holds a letter outside A, C, G, T"""
    __slots__ = ("family", "label", "seq", "m", "row", "strand", "clean", "special", "tpl")

    def interior(self, n):
        return self.seq[n:len(self.seq) - n] if len(self.seq) > 2 * n else ""


class Builder(object):
    def __init__(self, layouts, t5, t3, n, seed):
        self.layouts, self.t5, self.t3, self.n = layouts, t5, t3, n
        self.rng = random.Random(seed)
        self.reads = []

    def acgt(self, k):
        return [self.rng.choice("ACGT") for _ in range(k)]

    def other(self, c):
        return self.rng.choice([x for x in "ACGT" if x != c.upper()])

    def copy(self, tpl, bsubs, fsubs=0, insertion=False):
        """template `tpl` with barcodes drawn at random: `bsubs` substitutions in every barcode, `fsubs` in the flanks,
        `insertion`: one more letter in the middle of the first barcode (a gap of cost 1: the raw barcode score changes
        parity, which substitutions at 2 apiece never do)"""
        lay = self.layouts[tpl]
        seq = list(synth.fill(lay, self.rng.randrange(1 << 16), self.rng.randrange(1 << 16)))
        spans = [range(p.start, p.end + 1) for p in (lay.barcode_pos_1, lay.barcode_pos_2) if p.end >= 0 and p.start >= 0]
        inside = set(i for s in spans for i in s)
        for s in spans:
            for p in self.rng.sample(list(s), min(bsubs, len(s))):
                seq[p] = self.other(seq[p])
        for p in self.rng.sample([i for i in range(len(seq)) if i not in inside], fsubs):
            seq[p] = self.other(seq[p])
        if insertion:
            seq.insert(spans[0][len(spans[0]) // 2], self.rng.choice("ACGT"))
        return seq

    def add(self, family, label, m, row, strand="+", tpl=None, bsubs=0, fsubs=0, insertion=False, letters=None):
        """END5 + interior of m letters + END3 with a copy that ends at interior row `row` of `strand`.  What the copy has
        outside the interior goes into the windows' random padding, never over the end adapters.  `letters`: (offset from
        `row`, text) written over the finished interior on the same strand (text "lower": ten letters in lower case)."""
        rng, n, lays = self.rng, self.n, self.layouts
        tpl = self.t5 if tpl is None else tpl
        b, b2 = rng.randrange(1 << 16), rng.randrange(1 << 16)
        a5 = list(synth.fill(lays[self.t5], b, b2))
        a3 = list(synth.revcomp_acgt(synth.fill(lays[self.t3], b, b2)))
        assert LEAD + len(a5) <= n and LEAD + len(a3) <= n
        canvas = self.acgt(LEAD) + a5 + self.acgt(n - LEAD - len(a5)) + self.acgt(m) + self.acgt(n - LEAD - len(a3)) + a3 + self.acgt(LEAD)
        total = len(canvas)
        lo, hi = LEAD + len(a5) + 2, total - LEAD - len(a3) - 2            # what may be written over
        cp = self.copy(tpl, bsubs, fsubs, insertion)

        def put(j, c):
            pos = n + j if strand == "+" else total - n - 1 - j
            if lo <= pos < hi:
                canvas[pos] = c if strand == "+" else utils.revcomp(c)
                return True
            return False
        whole = True
        for i, c in enumerate(cp):
            j = row - len(cp) + 1 + i
            whole = put(j, c) and 0 <= j < m and whole
        if letters:
            off, text = letters
            for i in range(10 if text == "lower" else len(text)):
                j = row + off + i
                assert 0 <= j < m, (label, j, m)
                pos = n + j if strand == "+" else total - n - 1 - j
                canvas[pos] = canvas[pos].lower() if text == "lower" else text[i]
        r = Read()
        r.family, r.label, r.seq, r.m, r.row, r.strand, r.tpl = family, label, "".join(canvas), m, row, strand, tpl
        r.clean = whole and fsubs == 0 and not insertion and not letters
        r.special = any(c not in "ACGTacgt" for c in r.interior(n))
        assert len(r.seq) == 2 * n + m
        self.reads.append(r)
        return r


def subs_levels(blen):
    """substitutions per barcode: one, a quarter, and four levels up to half of it (where the score crosses 50)"""
    h = blen // 2
    return (1, blen // 4, h - 3, h - 2, h - 1, h)


def build(spec, layouts, n, families, seed, filler=120, context=11):
    """the constructed reads of one plan; `families`: which of 0 .. 5 (6, the end of the packed path, is long_reads())"""
    b = Builder(layouts, spec["t5"], spec["t3"], n, seed)
    lens = sorted({len(layouts[t].get_adapter_sequences()) for t in (spec["t5"], spec["t3"])})
    tl = len(layouts[spec["t5"]].get_adapter_sequences())
    blen = layouts[spec["t5"]].get_barcode_length(0)
    levels = subs_levels(blen)
    k = [0]

    def each(family, label, m, row, strands="+-", subs=None, tpl=None, **kw):
        """one read per strand and substitution level; the copy is the 5' template, every third time the 3' one, unless `tpl` says which"""
        for strand in strands:
            for s in (levels if subs is None else subs):
                k[0] += 1
                t = tpl if tpl is not None else spec["t3" if k[0] % 3 == 0 else "t5"]
                b.add(family, "%s %s s%d" % (label, strand, s), m, row, strand=strand, tpl=t, bsubs=s, **kw)
    if 1 in families:
        # the copy ends on either side of the binary16 kernel's block boundaries (rows 152 k) ...
        for row in (150, 151, 152, 153, 154, 303, 304, 305):
            each(1, "end row %d" % row, row + 1 + b.rng.randrange(120), row)
        # ... lies across them, with the boundary inside the leading flank's adapter letters, inside the barcode ...
        bc_mid = layouts[spec["t5"]].barcode_pos_1.start + blen // 2
        for edge in (PK_ROWS, 2 * PK_ROWS):
            for cut, what in ((3, "adapter"), (bc_mid, "barcode")):
                row = edge - 1 + (tl - cut)                          # the copy's letter `cut` is the first of the next block
                each(1, "row %d inside the %s" % (edge, what), row + 1 + b.rng.randrange(120), row, tpl=spec["t5"])
        # ... and far down: block 20 and later (the DP row has been re-based twenty times by then)
        for row in (20 * PK_ROWS - 1, 20 * PK_ROWS, 20 * PK_ROWS + tl // 2, 23 * PK_ROWS + 70):
            each(1, "block 20+, end row %d" % row, row + 1 + b.rng.randrange(200), row, subs=levels[1::2])
    if 2 in families:
        # interior lengths around the template lengths, the length classes and the blocks: the copy ends at the last row
        # (an interior shorter than the copy holds its tail only)
        # (0: no interior at all, which the reference scores like a scan that finds no barcode -- 0.0, a hit at rung 0 only)
        ms = {0, 1, 2, 63, 64, 65, 127, 128, 129, 151, 152, 153, 303, 304, 305}
        for t in lens:
            ms |= {t - 1, t, t + 1}
        for m in sorted(ms):
            each(2, "m %d" % m, m, m - 1 if m < 2 * max(lens) else m - 1 - b.rng.randrange(m - max(lens)), subs=levels[2::3])
        # two interiors of one length class, 63 rows apart, each with its hit in its own last row
        for c in (1, 2, 4, 7):
            for m in (MID_CLASS_ROWS * c + 1, MID_CLASS_ROWS * c + MID_CLASS_ROWS):
                each(2, "class %d, m %d, hit in the last row" % (c, m), m, m - 1, subs=levels[1::3])
    if 3 in families:
        m = 200
        for cut in (1, 5, 20):                                       # the copy's first letters lie in the window in front
            each(3, "cut by the start, %d letters" % cut, m, tl - cut - 1, tpl=spec["t5"])
        for back in (1, 2):
            each(3, "ends at row m - %d" % back, m, m - back)
        bc_end = layouts[spec["t5"]].barcode_pos_1.end
        for past in (1, 5, 12):                                      # the barcode's last letters lie in the window behind
            each(3, "barcode %d past the end" % past, m, m - 1 + past + (tl - 1 - bc_end), tpl=spec["t5"])
    if 4 in families:
        # substitutions in the flanks: at or below region_min_adapter_score the barcode is searched in the first window
        # of the interior -- with the copy inside it, and beyond it
        for row, where in ((100, "inside the first window"), (400, "beyond the first window")):
            for f in (0, 1, 2, 3, 5):
                each(4, "%d flank substitutions, copy %s" % (f, where), 520, row, subs=(0, levels[3], levels[5]), fsubs=f)
    if 5 in families:
        for text in ("N", "NNNNNNN", "R", "lower"):
            for off, where in ((-tl // 2, "inside the copy"), (1, "behind the copy"), (170, "in another block")):
                each(5, "%s %s" % (text, where), 520, 200, subs=(1, levels[4]), letters=(off, text))
            each(5, "neighbour of %s" % text, 520, 200, subs=(1, levels[4]))
    if 0 in families:
        # filler at the decision: half a barcode of substitutions, with and without an inserted letter, anywhere
        for i in range(filler):
            m = 60 + b.rng.randrange(700)
            row = min(m - 1, max(lens) + b.rng.randrange(max(1, m - max(lens))))
            b.add(0, "decision %d" % i, m, row, strand="+-"[i % 2], tpl=(spec["t5"], spec["t3"])[i // 2 % 2],
                  bsubs=levels[(4 + i % 2) if spec["mode"] == "dual" else (3 + i % 3)], insertion=bool(i // 4 % 2))
        # (the dual kit's verdict is the smaller of two scores: one level more damage puts it at the decision as often)
        # ... and interiors that hold nothing but the first letters of a barcode, as many as the decision needs and one fewer
        # (against a set of 96 no substituted copy scores that low: some other barcode of the set fits it better)
        # (not for the dual kit: its verdict is the smaller of two scores, and such an interior holds one barcode)
        bc_end = layouts[spec["t5"]].barcode_pos_1.end
        for t in () if spec["mode"] == "dual" else target_lengths([layouts[spec["t5"]], layouts[spec["t3"]]], spec["mode"], context):
            for m in (decision_raw(t) - 1, decision_raw(t)):
                for i in range(24):
                    b.add(0, "%d barcode letters" % m, m, m - 1 + (tl - 1 - bc_end), strand="+-"[i % 2], tpl=spec["t5"])
    return b.reads


def long_reads(spec, layouts, n, seed):
    """family 6: interiors of 16 383, 16 384 (the last of the packed path) and 16 385 letters (the first of the one-wave /
    general kernels), the copy near the start, near the end and in the last row (for 16 385: across row 16 384)"""
    b = Builder(layouts, spec["t5"], spec["t3"], n, seed)
    tl = len(layouts[spec["t5"]].get_adapter_sequences())
    levels = subs_levels(layouts[spec["t5"]].get_barcode_length(0))
    for m in (MID_MAX - 1, MID_MAX, MID_MAX + 1):
        for row, where in ((tl + 60, "near the start"), (m - 40, "near the end"), (m - 1, "in the last row")):
            for i, strand in enumerate("+-"):
                b.add(6, "m %d, copy %s %s" % (m, where, strand), m, row, strand=strand, tpl=spec["t5"], bsubs=levels[(3, 5)[i ^ (row & 1)]])
    for i in range(6):                                               # ordinary interiors beside them
        b.add(0, "ordinary %d" % i, 300 + 50 * i, 200, strand="+-"[i % 2], bsubs=levels[3 + i % 3], insertion=bool(i % 2))
    return b.reads


# ---- the expected side ---------------------------------------------------------------------------------------------------------
def target_lengths(layouts, mode, context):
    """lengths of the barcode targets (context + barcode + context) of `layouts`"""
    out = set()
    for lay in layouts:
        for s in range(2 if mode == "dual" else 1):
            bs = lay.get_barcode_set(s)
            if bs:
                out.add(len(lay.get_upstream_context(context, s)) + len(bs[0].sequence) + len(lay.get_downstream_context(context, s)))
    return sorted(out)


def decision_raw(den):
    """the smallest raw score r with r * 100.0 / den >= 50.0, in the arithmetic of the scan"""
    return next(r for r in range(-1, 4097) if not r * 100.0 / (1.0 * den) < 50.0)


class Plan(object):
    """one (kit, scoring, R1 rule, reads): the oracle's records without any 997 and with every called read 997, the interior
    score of every read, the ladder and the staircase levels.  Computed once, shared by every test and path."""

    def __init__(self, kit_name, cfg_name="default", rule=native.R1_STRIPED, families=None, long=False, threads=8):
        spec = KITS[kit_name]
        self.name = "%s/%s/%s%s" % (kit_name, cfg_name, "scalar" if rule == native.R1_SCALAR else "striped", "/long" if long else "")
        self.kit_name, self.cfg_name, self.rule, self.spec, self.threads = kit_name, cfg_name, rule, spec, threads
        self.cfg = scoring(cfg_name)
        self.n = int(self.cfg.max_align_length)
        self.mode = spec["mode"]
        self.layouts = scanner.factory(mode=spec["mode"], kit=spec["kit"], scan_middle_adapter=True).layouts
        if families is None:
            families = (0, 1, 2, 3, 4, 5) if spec["families"] == "all" and cfg_name == "default" else (0, 1, 2, 3)
        seed = 1000 + sorted(KITS).index(kit_name)
        self.cases = long_reads(spec, self.layouts, self.n, seed) if long else build(spec, self.layouts, self.n, families, seed, filler=650 if 5 in families else 300 if self.mode == "dual" else 120, context=int(self.cfg.barcode_context_length))
        self.reads = [c.seq for c in self.cases]
        self.packed = native.pack_reads(self.reads)
        self.family = np.array([c.family for c in self.cases])
        # the oracle without the interior's verdict, and with it for every called read
        self.base, self.base_cnt = oracle_lib.scan(self.descriptor(1e9), packed=self.packed, counts=True, threads=threads)
        self.all997 = oracle_lib.scan(self.descriptor(-1e9), packed=self.packed, threads=threads)
        self.called = self.base["adapter_idx"] >= 0
        assert not (self.base["exit_status"] == 997).any()
        assert ((self.all997["exit_status"] == 997) == self.called).all()
        # the interior's scan on both strands, with the templates of the called kit (scanner_base.py:479-519)
        nr = len(self.reads)
        self.fwd = np.zeros(nr, dtype=native.RESULT_DTYPE)
        self.rev = np.zeros(nr, dtype=native.RESULT_DTYPE)
        self.wraps = np.zeros(nr, dtype=bool)
        self.kits_called = sorted({self.layouts[a].kit for a in self.base["adapter_idx"][self.called]})
        for kit in self.kits_called:
            idx = [i for i in range(nr) if self.called[i] and self.layouts[self.base["adapter_idx"][i]].kit == kit]
            sub = self.sub_descriptor(kit)
            mids = [self.cases[i].interior(self.n) for i in idx]
            self.fwd[idx], tf = oracle_lib.scan_sequences(sub, mids, trace=True)
            self.rev[idx], tr = oracle_lib.scan_sequences(sub, [utils.revcomp(s) for s in mids], trace=True)
            # rule R4: a barcode region whose start wraps around comes out longer than a window (on either strand, in
            # any set): the packed interior scan hands such a read on, as it does an interior beyond its last length class
            sets = 2 if self.mode == "dual" else 1
            self.wraps[idx] = ((tf["region_len"][:, :sets] > self.n) | (tr["region_len"][:, :sets] > self.n)).any(axis=1)
        self.derive()

    def descriptor(self, threshold, layouts=None):
        d = native.KitDescriptor(self.layouts if layouts is None else layouts, self.cfg, mode=self.mode, ends=native.ENDS_BOTH,
                                 scan_middle=layouts is None, r1_rule=self.rule)
        d.desc.middle_min_score = float(threshold)
        return d

    def sub_descriptor(self, kit):
        return self.descriptor(50.0, layouts=[lay for lay in self.layouts if lay.kit == kit])

    def derive(self, raw_bump=None):
        """scores, ladder and levels from the two strands' records; `raw_bump`: array added to both strands' raw scores
        (the sensitivity runs of the profile: the comparison must then fail)"""
        def score(recs):
            raw = recs["raw_score"].astype(np.int64) + (0 if raw_bump is None else raw_bump)
            return raw * 100.0 / (1.0 * recs["score_den"].astype(np.int64)), raw
        (sf, rf), (sr, rr) = score(self.fwd), score(self.rev)
        use_rev = sr > sf
        self.score = np.where(self.called, np.where(use_rev, sr, sf), -np.inf)
        self.raw = np.where(use_rev, rr, rf)
        self.den = np.where(use_rev, self.rev["score_den"], self.fwd["score_den"]).astype(np.int64)
        lays = [lay for lay in self.layouts if lay.kit in self.kits_called]
        self.tlens = target_lengths(lays, self.mode, int(self.cfg.barcode_context_length))
        rungs = {0.0, (max(self.tlens) + 1) * 100.0 / (1.0 * max(self.tlens))}
        for t in self.tlens:
            rungs |= {r * 100.0 / (1.0 * t) for r in range(1, t + 1)}
        self.ladder = np.array(sorted(rungs))
        self.level = np.searchsorted(self.ladder, self.score, side="right")          # rungs at which the read is 997

    def adjacent(self):
        """the rungs next to a score that occurs: each occurring score's own rung and the one above it"""
        lv = self.level[self.called]
        top = len(self.ladder) - 1
        return sorted(set(np.clip(lv - 1, 0, top)) | set(np.clip(lv, 0, top)))

    def hits(self, i):
        return self.called & (self.level > i)

    def expected(self, i):
        """(records, counts) at rung i: the oracle's records with the 997 bit from the interior scores"""
        hit = self.hits(i)
        recs = self.base.copy()
        recs[hit] = self.all997[hit]
        return recs, self.counts_of(hit)

    def counts_of(self, hit):
        """the count vector with the reads `hit` void: [barcodes.., none][kits.., none][skipped] (helpers.driver_histogram)"""
        if not hasattr(self, "_slots"):
            d = self.descriptor(50.0)
            nb, nk = len(d.slot_ids), len(d.kit_names)
            nbc = nb * nb if self.mode == "dual" else nb
            slot = np.full(len(self.reads), nbc, dtype=np.int64)
            kslot = np.full(len(self.reads), nbc + 1 + nk, dtype=np.int64)
            for i, rec in enumerate(self.base):
                if rec["adapter_idx"] >= 0:
                    lay = self.layouts[rec["adapter_idx"]]
                    kslot[i] = nbc + 1 + d.kit_slots[lay.kit]
                    if rec["barcode_idx"] >= 0:
                        slot[i] = d.id_slots[lay.get_barcode_set(0)[rec["barcode_idx"]].id]
                        if self.mode == "dual":
                            slot[i] = slot[i] * nb + d.id_slots[lay.get_barcode_set(1)[rec["barcode2_idx"]].id]
            self._slots = (slot, kslot, nbc, nbc + 1 + nk, d.n_count_buckets)
        slot, kslot, none, knone, nbuckets = self._slots
        return (np.bincount(np.where(hit, none, slot), minlength=nbuckets) + np.bincount(np.where(hit, knone, kslot), minlength=nbuckets)).astype(np.int64)

    def oracle_at(self, i):
        """the full oracle at rung i"""
        return oracle_lib.scan(self.descriptor(self.ladder[i]), packed=self.packed, counts=True, threads=self.threads)

    def adapter_score(self, case):
        """the oracle's normalised adapter score of `case`'s interior on the copy's strand (the templates of the kit, first best)"""
        mid = case.interior(self.n)
        if case.strand == "-":
            mid = utils.revcomp(mid)
        best = -1.0
        for lay in self.layouts:
            if lay.kit != self.layouts[self.spec["t5"]].kit:
                continue
            tpl = lay.get_adapter_sequences()
            nbc = tpl.count("N")
            den = (len(tpl) - nbc) * int(self.cfg.match) + nbc * int(self.cfg.nmatch)
            sc = oracle_lib.sg(mid, tpl, int(self.cfg.gap_open), int(self.cfg.gap_extend), self.cfg.matrix.table, rule=self.rule)[0]
            best = max(best, sc * 100.0 / den)
        return best

    def histogram(self):
        """{score: reads} of the called reads, as text"""
        vals, n = np.unique(self.score[self.called], return_counts=True)
        return " ".join("%.2f:%d" % (v, c) for v, c in zip(vals, n))


_plans = {}


def plan(kit_name, cfg_name="default", rule=native.R1_STRIPED, families=None, long=False):
    key = (kit_name, cfg_name, rule, families, long)
    if key not in _plans:
        _plans[key] = Plan(kit_name, cfg_name, rule, families, long)
    return _plans[key]


#: the plans of the sweep: name -> arguments of plan()
PLANS = {
    "NBD": ("NBD",),
    "NBD-scalar": ("NBD", "default", native.R1_SCALAR, (0, 3)),
    "NBD-gap1": ("NBD", "gap1"),
    "NBD-n100": ("NBD", "n100"),
    "NBD-ext0": ("NBD", "ext0", native.R1_STRIPED, (0, 1, 3)),
    "PBC096": ("PBC096",),
    "DUAL": ("DUAL",),
    "AUTO": ("AUTO",),
}
LONG = ("NBD", "default", native.R1_STRIPED, None, True)


# ---- device paths ------------------------------------------------------------------------------------------------------------
#: path -> library options.  The interior's adapter scan runs bit-sliced from MIDDLE_ABS_MIN slots (by default a big tile
#: of 2048 per compute unit: never at this size), so the bit-sliced forms are forced and "no_abs" forces them and switches them off again
PATHS = {
    "default": {"NO_TINY": None},
    "no_bitslice": {"MIDDLE_NO_BITSLICE": 1},
    "abs_pipeline": {"MIDDLE_ABS_MIN": 1, "MIDDLE_ABS_ONE_WAVE": 0},
    "abs_one_wave": {"MIDDLE_ABS_MIN": 1, "MIDDLE_ABS_ONE_WAVE": 1},
    "abs_windows_from_reads": {"MIDDLE_ABS_MIN": 1, "MIDDLE_ABS_WINDOWS": 0},
    "no_abs": {"MIDDLE_ABS_MIN": 1, "MIDDLE_NO_ABS": 1},
    "generic": {"MIDDLE_GENERIC": 1},
}
#: (MIDDLE_NO_BITSLICE and MIDDLE_ABS_WINDOWS are A/B switches, csrc/options.h: a default build folds them away and has no such
#: path -- the sweep reports those two as skipped there; a build with -DQCAT_AB lists them, and the sweep then runs them too)
#: the paths that sweep the rungs next to an occurring score instead of the whole ladder: the general kernel walks every
#: interior on one lane (on an MI355X 2 .. 8 s per plan for a whole ladder and 20 s for the dual kit; 1.3 .. 5.9 s and 14 s
#: on these rungs; the module as a whole takes 93 s, profiles/middle_boundary_sweep.txt)
ADJACENT_ONLY = ("generic",)


def available(opts):
    """does the library list every option of `opts`?"""
    try:
        lib = native.HipLibrary.get().lib
    except (RuntimeError, OSError):
        return True                          # (no library: the tests say so when they run)
    return all(lib.qcat_get_option(name.encode(), None) >= 0 for name in opts)


#: for the reads around the end of the packed path: the one-wave kernels (the product's default) and the general kernel
LONG_PATHS = {
    "default": {"NO_TINY": None},
    "no_one_wave": {"NO_TINY": 1},
    "abs_pipeline": {"NO_TINY": None, "MIDDLE_ABS_MIN": 1, "MIDDLE_ABS_ONE_WAVE": 0},
    "generic": {"NO_TINY": None, "MIDDLE_GENERIC": 1},
}


def middle_tiles(ctx):
    tiles = (C.c_uint32 * 4)()
    native.HipLibrary.get().check(gc.lib().qcat_ctx_middle_bitslice_tiles(ctx.handle, tiles))
    return list(tiles)


def proof(p, path, opts, info, ran, tiles, wave_reads):
    """why `path` did not run what it is for (None: it did).  `info`: describe() of the kit; `ran`: the timing ring's marks;
    `tiles`: qcat_ctx_middle_bitslice_tiles -- big tiles walked bit-sliced, big tiles, tiles of 128 handed back to the
    binary16 kernel, tiles of 128; `wave_reads`: qcat_ctx_middle_wave_reads"""
    if "k_scan_middle" not in ran:
        return "no interior scan"
    packed = info["packed"] == 1 and info["adapter_f16"] == 1 and path != "generic"
    if ("k_middle_packed" in ran) != packed:
        return "packed interior scan %s" % ("missing" if packed else "ran")
    # the one-wave kernels take what the packed interior scan hands on: interiors beyond its last length class, and the
    # reads whose barcode region wraps around to more than a window (rule R4; from the oracle's traces of both strands)
    handed_on = int((p.called & ((np.array([c.m for c in p.cases]) > MID_MAX) | p.wraps)).sum())
    waves_on = packed and p.cfg.gap_open == p.cfg.gap_extend and opts.get("NO_TINY", 1) is None
    if wave_reads != (handed_on if waves_on else 0):
        return "one-wave interior kernels took %d reads, the packed interior scan hands on %d" % (wave_reads, handed_on)
    bit_sliced = packed and path.startswith("abs") and (info["bitslice_templates"] & 0xFF) == info["n_templates"]
    if not bit_sliced:
        return None if tiles == [0, 0, 0, 0] else "bit-sliced interior adapter scan ran"
    if not (tiles[0] >= 1 and tiles[1] >= tiles[0] and tiles[3] > tiles[2]):
        return "bit-sliced interior adapter scan did not run"
    special = bool((p.called & np.array([c.special for c in p.cases])).any())
    if (special and not tiles[2]) or (tiles[2] and not special and len(p.kits_called) == 1):
        return "tiles handed back to the binary16 kernel: %d" % tiles[2]
    return None



def sweep(p, path, rungs, setter, paths=PATHS):
    """scan p's reads on `path` under every rung of `rungs`: -> (problems, proofs): what differs from the expected records
    and counts, in words that name the reads' cases and their expected and observed staircase levels; the proof counters per rung"""
    opts = paths[path]
    ctx = gc.context()
    bases, offsets = p.packed
    saved = {name: native.get_option(name) for name in opts}
    setter(**opts)
    got_hit = {}
    bad, problems, proofs = {}, [], []
    try:
        for i in rungs:
            d = p.descriptor(p.ladder[i])
            kit = native.NativeKit(d)
            gc.ring(ctx)
            cnt = np.zeros(d.n_count_buckets, dtype=np.int64)
            recs = ctx.scan(kit, bases, offsets, counts=cnt)
            ran, tiles, waves = gc.ring(ctx), middle_tiles(ctx), int(gc.lib().qcat_ctx_middle_wave_reads(ctx.handle))
            why = proof(p, path, opts, kit.describe(), ran, tiles, waves)
            proofs.append((i, ran, tiles, waves))
            if why:
                problems.append("rung %d: path did not run: %s (ring %s, tiles %s, wave reads %d)" % (i, why, ran, tiles, waves))
            want, want_cnt = p.expected(i)
            got_hit[i] = recs["exit_status"] == 997
            if recs.tobytes() != want.tobytes():
                for r in np.nonzero(recs != want)[0]:
                    bad.setdefault(int(r), []).append(i)
            if not np.array_equal(cnt, want_cnt):
                problems.append("rung %d (%.4f): counts differ at buckets %s" % (i, p.ladder[i], np.nonzero(cnt != want_cnt)[0][:6]))
    finally:
        setter(**saved)
    for r in sorted(bad)[:8]:
        at = [i for i in rungs if got_hit[i][r]]
        observed = "997 at no rung" if not at else "997 up to rung %d (%.4f)" % (max(at), p.ladder[max(at)])
        lv = int(p.level[r])
        problems.append("read %d [%s, m %d, row %d]: expected level %d (score %.4f = %d / %d, 997 up to rung %d), observed %s; records differ at rungs %s"
                        % (r, p.cases[r].label, p.cases[r].m, p.cases[r].row, lv, p.score[r], p.raw[r], p.den[r], lv - 1, observed, bad[r][:6]))
    if len(bad) > 8:
        problems.append("... and %d more reads" % (len(bad) - 8))
    return problems, proofs
