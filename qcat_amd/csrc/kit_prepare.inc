// kit_prepare.inc -- host-side validation and flattening of a qcat_kit_desc (see kit.h).
// Included by qcat_hip.hip.

namespace qk {

static inline int smallest_raw(double mul_den, double threshold, bool strict) {
    // smallest integer raw in [-4096, 4096] with raw*100.0/den (>|>=) threshold; the map is
    // increasing in raw because den > 0.
    for (int raw = -4096; raw <= 4096; ++raw) {
        double s = raw * 100.0 / mul_den;
        if (strict ? (s > threshold) : (s >= threshold)) return raw;
    }
    return RAW_NEVER;
}

// biased substitution score of the packed fast path: W' = max(W + 2g, 0) (exact for linear
// gaps: a diagonal step can never be worse than gap+gap), PAD rows get W' = 0.
static inline int biased_w(const int8_t* mat, int tcode, int qcode, int g) {
    if (qcode == QCAT_CODE_PAD) return 0;
    int w = mat[tcode * 7 + qcode] + 2 * g;
    return w < 0 ? 0 : w;
}

// High byte of the binary16 encoding of the integer v, or -1 when the low byte is not zero (the
// fp16-lane barcode kernels look scores up one byte per half with v_perm_b32).  Admissible:
// 0..8, 10, 12, 14, 16, 20, 24, 28, 32, ...
static inline int f16_high_byte(int v) {
    if (v < 0 || v > 2048) return -1;
    if (v == 0) return 0;
    int e = 0;
    while ((v >> (e + 1)) != 0) ++e;
    const int num = (v - (1 << e)) * 1024;
    if (num % (1 << e)) return -1;
    const int bits = ((e + 15) << 10) | (num >> e);
    return (bits & 0xFF) ? -1 : (bits >> 8);
}

// binary16 bits of a small non-negative integer (exact up to 2048)
static inline uint16_t f16_bits(int v) {
    if (v <= 0) return 0;
    int e = 0;
    while ((v >> (e + 1)) != 0) ++e;
    const int mant = e <= 10 ? ((v - (1 << e)) << (10 - e)) : ((v - (1 << e)) >> (e - 10));
    return (uint16_t)(((e + 15) << 10) | mant);
}

// Build fast tables for one target (codes t[0..m)): one dword per column holding
// W'(A|T|G|C, t_j); checks that the "special" query codes (N, X, other) score the same against
// every column, returning that shared pool through *special (0xFFFFFFFF = not yet set).
static bool build_fast_tables(const int8_t* mat, const uint8_t* t, int m, int g,
                              uint32_t* out, uint32_t* special, int width, bool f16 = false) {
    // right-aligned in `width` dwords; the left padding is all-zero (score 0 for every query code)
    for (int j = 0; j < width - m; ++j) out[j] = 0;
    out += width - m;
    for (int j = 0; j < m; ++j) {
        uint32_t w = 0;
        for (int q = 0; q < 4; ++q) {
            int v = biased_w(mat, t[j], q, g);
            if (f16) v = f16_high_byte(v);
            if (v < 0 || v > 255) return false;
            w |= (uint32_t)v << (8 * q);
        }
        out[j] = w;
        uint32_t sp = 0;
        for (int q = 4; q < 8; ++q) {
            int v = biased_w(mat, t[j], q, g);
            if (f16) v = f16_high_byte(v);
            if (v < 0 || v > 255) return false;
            sp |= (uint32_t)v << (8 * (q - 4));
        }
        if (*special == 0xFFFFFFFFu) *special = sp;
        else if (*special != sp) return false;
    }
    return true;
}

int kit_prepare(const qcat_kit_desc* d, HostKit* hk, std::string* err) {
    auto fail = [&](int rc, const std::string& m) { *err = m; return rc; };
    if (!d) return fail(QCAT_ERR_ARG, "null kit descriptor");
    if (d->abi_version != QCAT_ABI_VERSION) return fail(QCAT_ERR_ARG, "kit descriptor ABI version mismatch");
    if (d->mode != QCAT_MODE_EPI2ME && d->mode != QCAT_MODE_DUAL && d->mode != QCAT_MODE_SIMPLE) return fail(QCAT_ERR_ARG, "invalid mode");
    const bool simple = d->mode == QCAT_MODE_SIMPLE;
    if (simple && d->n_templates != 1) return fail(QCAT_ERR_ARG, "simple mode takes exactly one (empty) template holding the barcode list");
    if (d->ends != QCAT_ENDS_5P && d->ends != QCAT_ENDS_BOTH) return fail(QCAT_ERR_ARG, "invalid ends mask");
    if (d->n_templates < 1 || d->n_templates > MAX_T || !d->templates)
        return fail(QCAT_ERR_ARG, "kit needs 1.." + std::to_string(MAX_T) + " adapter templates");
    if (d->max_align_length < 1 || d->max_align_length > MAX_WIN)
        return fail(QCAT_ERR_UNSUPPORTED, "max_align_length must be in 1.." + std::to_string(MAX_WIN));
    if (d->gap_open < 0 || d->gap_extend < 0) return fail(QCAT_ERR_ARG, "negative gap penalty");
    if (d->n_barcode_slots < 1 || d->n_kit_slots < 1) return fail(QCAT_ERR_ARG, "slot counts must be positive");
    if (d->mode == QCAT_MODE_DUAL && (int64_t)d->n_barcode_slots * d->n_barcode_slots > (1 << 24))
        return fail(QCAT_ERR_UNSUPPORTED, "too many dual barcode count buckets");

    DevKit& k = hk->dk;
    memset(&k, 0, sizeof k);
    hk->codes.clear(); hk->ids.clear(); hk->tables.clear(); hk->ascii.clear(); hk->simple_packed = 0;
    k.mode = d->mode; k.ends = d->ends; k.nt = d->n_templates;
    k.gap_open = d->gap_open; k.gap_extend = d->gap_extend;
    k.max_align = d->max_align_length; k.ext = d->extracted_barcode_extension;
    k.n_barcode_slots = d->n_barcode_slots; k.n_kit_slots = d->n_kit_slots;
    k.scan_middle = (d->scan_middle_adapter && d->ends == QCAT_ENDS_BOTH) ? 1 : 0;
    k.middle_hits_empty = smallest_raw(1.0, d->middle_min_score, false) <= 0 ? 1 : 0;     // (0 * 100.0 / tlen >= middle_min_score)
    k.n_buckets = ((d->mode == QCAT_MODE_DUAL) ? d->n_barcode_slots * d->n_barcode_slots : d->n_barcode_slots)
                  + 1 + d->n_kit_slots + 1 + 1;              // [barcodes.., none][kits.., none][skipped]
    k.min_read_length = d->min_read_length > 0 ? d->min_read_length : 0;
    k.trim_reads = d->trim_reads ? 1 : 0;
    if (d->r1_rule != QCAT_R1_STRIPED && d->r1_rule != QCAT_R1_SCALAR) return fail(QCAT_ERR_ARG, "r1_rule must be QCAT_R1_STRIPED or QCAT_R1_SCALAR");
    k.r1_scalar = d->r1_rule == QCAT_R1_SCALAR ? 1 : 0;
    memcpy(k.amat, d->adapter_matrix, 49);
    memcpy(k.bmat, d->barcode_matrix, 49);

    bool fast = (d->gap_open == d->gap_extend) && d->max_align_length <= 150 && !simple;
    uint32_t sp_adapter = 0xFFFFFFFFu, sp_barcode = 0xFFFFFFFFu;
    const int ga = d->gap_open;       // adapter gap (linear only on the fast path)
    const int gb = 1;                 // barcode alignments: open = extend = 1 (scanner_base.py:115-116)
    // fp16-lane barcode kernels need every biased barcode score to be a binary16 value whose low
    // byte is zero (true for the reference's +1/-1 matrix: 3, 1, 2, 0); otherwise the u16 kernels run
    bool bf16ok = !opt_on(QO_BARCODE_U16);
    {
        int maxwb = 0;
        for (int tc = 0; tc < 7 && bf16ok; ++tc)
            for (int qc = 0; qc < 8; ++qc) {
                const int v = biased_w(d->barcode_matrix, tc, qc, gb);
                if (v > maxwb) maxwb = v;
                if (f16_high_byte(v) < 0) { bf16ok = false; break; }
            }
        // every value of the biased DP must stay an exactly representable integer (< 2048)
        if ((int64_t)maxwb * MAX_TARGET + (int64_t)gb * (MAX_WIN + MAX_TARGET) > 2047) bf16ok = false;
    }

    for (int t = 0; t < k.nt; ++t) {
        const qcat_template_desc& s = d->templates[t];
        DevTpl& p = k.tpl[t];
        if (simple ? s.length != 0 : (!s.sequence || s.length < 1 || s.length > MAX_TLEN))
            return fail(QCAT_ERR_ARG, simple ? std::string("simple mode: the template must be empty")
                                             : "template " + std::to_string(t) + ": length must be in 1.." + std::to_string(MAX_TLEN));
        if (s.kit_slot < 0 || s.kit_slot >= d->n_kit_slots) return fail(QCAT_ERR_ARG, "template kit_slot out of range");
        p.len = s.length; p.trim_offset = s.trim_offset; p.is_double = s.is_double_barcode ? 1 : 0;
        p.kit_slot = s.kit_slot;
        p.code_off = (int32_t)hk->codes.size();
        hk->ascii_tpl_off[t] = (int32_t)hk->ascii.size();
        for (int j = 0; j < p.len; ++j) {
            hk->codes.push_back(code_of_ascii((uint8_t)s.sequence[j]));
            hk->ascii.push_back(s.sequence[j]);
        }
        int bc_total = 0;
        for (int i = 0; i < 2; ++i) {
            p.bc_end[i] = s.bc_end[i]; p.bc_len[i] = s.bc_len[i];
            hk->bc_start[t][i] = s.bc_start[i];
            bc_total += s.bc_len[i];
            if (s.bc_len[i] < 0 || (simple ? s.bc_end[i] != -1 : s.bc_end[i] >= p.len)) return fail(QCAT_ERR_ARG, "template placeholder out of range");
        }
        p.den = simple ? 1 : (p.len - bc_total) * d->match + bc_total * d->nmatch;      // scanner_base.py:308-310
        if (p.den <= 0)
            return fail(QCAT_ERR_UNSUPPORTED, "template " + std::to_string(t) +
                        ": non-positive normalisation denominator (" + std::to_string(p.den) + ")");
        p.region_min_raw = smallest_raw((double)p.den, d->region_min_adapter_score, true);
        // fast adapter tables
        p.tbl_off = -1; p.static_kernel = -1; p.fused_kernel = -1; p.fused_partner = -1; p.abs_jit = 0;
        p.width = adapter_width_class(p.len);
        if (fast && p.width) {
            size_t off = hk->tables.size();
            hk->tables.resize(off + p.width);
            uint32_t sp = sp_adapter;
            if (build_fast_tables(k.amat, &hk->codes[p.code_off], p.len, ga, &hk->tables[off], &sp, p.width)) {
                sp_adapter = sp; p.tbl_off = (int32_t)off;
            } else {
                hk->tables.resize(off);
            }
        }
        if (p.tbl_off < 0) fast = false;

        for (int i = 0; i < 2; ++i) {
            const qcat_barcode_set_desc& bs = s.sets[i];
            DevSet& q = p.sets[i];
            memset(&q, 0, sizeof q);
            q.tbl_off = -1; q.static_kernel = -1; q.case_off = 0; q.n_pairs = 0; q.quad_off = 0; q.n_quads = 0; q.bs_off = -1; q.hot_len = 0; q.bs_short_min = 0; q.bs_kernel = -1; q.bs_case_off = 0; q.len_off = -1;
            hk->ascii_set_off[t][i] = -1;
            if (bs.n <= 0) continue;
            if (bs.n > QCAT_MAX_BARCODES) return fail(QCAT_ERR_UNSUPPORTED, "barcode set too large");
            if (!bs.sequences || !bs.ids || bs.barcode_len < 1) return fail(QCAT_ERR_ARG, "bad barcode set");
            if (bs.barcode_len != s.bc_len[i])
                return fail(QCAT_ERR_ARG, "Adapter length does not match place holder length");   // layout.py:55-61
            // `sequences` is a NUL-terminated string of n * barcode_len characters: a shorter one (barcodes of
            // unequal length packed by a careless caller) would be read past its end below
            if (strnlen(bs.sequences, (size_t)bs.n * bs.barcode_len) != (size_t)bs.n * bs.barcode_len)
                return fail(QCAT_ERR_ARG, "barcode set: sequences is shorter than n * barcode_len");
            q.n = bs.n; q.blen = bs.barcode_len;
            // barcodes of unequal length (ABI 4): a user FASTA in simple mode; each is aligned with its own length
            // (qcat/scanner_base.py:108-119).  Rows are padded to barcode_len with PAD codes the kernels never reach.
            bool ragged = false;
            if (bs.lengths) {
                for (int b = 0; b < bs.n; ++b) {
                    if (bs.lengths[b] < 1 || bs.lengths[b] > bs.barcode_len) return fail(QCAT_ERR_ARG, "barcode set: lengths[b] outside 1..barcode_len");
                    ragged = ragged || bs.lengths[b] != bs.barcode_len;
                }
            }
            if (ragged && !simple)
                return fail(QCAT_ERR_UNSUPPORTED, "barcodes of unequal length are covered in simple mode only (a template's placeholder has one length, layout.py:55-61)");
            int n = d->barcode_context_length, up0 = 0, up1 = 0, dn0 = 0, dn1 = 0;
            if (s.bc_end[i] > -1) {                                       // layout.py:191-238
                up0 = s.bc_start[i] - n; if (up0 < 0) up0 = 0;
                up1 = s.bc_start[i]; if (up1 < up0) up1 = up0;
                dn0 = s.bc_end[i] + 1;
                dn1 = s.bc_end[i] + n + 1; if (dn1 > p.len) dn1 = p.len;
                if (dn1 < dn0) dn1 = dn0;
            }
            q.uplen = up1 - up0; q.downlen = dn1 - dn0; q.tlen = q.uplen + q.blen + q.downlen;
            if (q.tlen < 1 || q.tlen > MAX_TARGET)
                return fail(QCAT_ERR_UNSUPPORTED, "barcode target length " + std::to_string(q.tlen) +
                            " outside 1.." + std::to_string(MAX_TARGET));
            q.tgt_off = (int32_t)hk->codes.size();
            q.ids_off = (int32_t)hk->ids.size();
            hk->ascii_set_off[t][i] = (int32_t)hk->ascii.size();
            for (int b = 0; b < q.n; ++b) {
                for (int j = 0; j < q.uplen; ++j) hk->codes.push_back(hk->codes[p.code_off + up0 + j]);
                const int own = ragged ? bs.lengths[b] : q.blen;
                for (int j = 0; j < q.blen; ++j) {
                    char c = bs.sequences[(size_t)b * q.blen + j];
                    hk->codes.push_back(j < own ? code_of_ascii((uint8_t)c) : (uint8_t)QCAT_CODE_PAD);
                    hk->ascii.push_back(c);
                }
                for (int j = 0; j < q.downlen; ++j) hk->codes.push_back(hk->codes[p.code_off + dn0 + j]);
                if (bs.ids[b] < 0 || bs.ids[b] >= d->n_barcode_slots) return fail(QCAT_ERR_ARG, "barcode id slot out of range");
                hk->ids.push_back(bs.ids[b]);
            }
            // bit-sliced kernels (kernels_bitslice.inc): plain targets, up to 128 barcodes; the longer context leads
            // (reversed alignment if that is the downstream one) and its first 0 / 4 / 8 / 11 columns are shared; the
            // other context's columns are shared through the reversed DP (bs_post)
            q.hot_len = q.blen + 2 * d->extracted_barcode_extension + 1;
            q.bs_pre = 0; q.bs_rev = 0; q.bs_post = 0; q.bs_short_min = q.hot_len; q.bs_kernel = -1; q.bs_case_off = 0;
            {
                q.bs_rev = q.downlen > q.uplen ? 1 : 0;
                const int lead = q.bs_rev ? q.downlen : q.uplen;
                q.bs_pre = lead >= 11 ? 11 : (lead >= 8 ? 8 : (lead >= 4 ? 4 : 0));
                q.bs_post = bs_post_of(q.bs_rev ? q.uplen : q.downlen, q.tlen, q.bs_pre);
                q.bs_short_min = (q.bs_post > 0 && q.hot_len != d->max_align_length) ? std::max(1, q.hot_len - BS_PAD_ROWS) : q.hot_len;
                const int own = q.tlen - q.bs_pre - q.bs_post;
                // (BS_MAX_TARGET: a target of 64 columns read without an error scores 64, one more than the counters' seven planes hold)
                bool plain = own >= BS_C_MIN && own <= BS_C_MAX && q.tlen <= BS_MAX_TARGET && q.n <= 128 && q.hot_len <= 150;
                for (size_t x = 0; x < (size_t)q.n * q.tlen && plain; ++x) plain = hk->codes[q.tgt_off + x] <= 3;
                if (plain) {
                    q.bs_off = (int32_t)hk->ids.size();
                    for (int b = 0; b < q.n; ++b) {
                        uint64_t l1 = 0, l0 = 0;
                        for (int j = 0; j < q.tlen; ++j) {               // bit j = column j in the order the kernel walks them
                            const uint8_t c = hk->codes[q.tgt_off + (size_t)b * q.tlen + (q.bs_rev ? q.tlen - 1 - j : j)];
                            l1 |= (uint64_t)((c >> 1) & 1) << j; l0 |= (uint64_t)(c & 1) << j;
                        }
                        hk->ids.push_back((int32_t)(uint32_t)l1); hk->ids.push_back((int32_t)(uint32_t)(l1 >> 32));
                        hk->ids.push_back((int32_t)(uint32_t)l0); hk->ids.push_back((int32_t)(uint32_t)(l0 >> 32));
                    }
                }
            }
            q.min_raw_pass = smallest_raw(1.0 * q.tlen, d->min_quality, false);
            q.min_raw_conflict = smallest_raw(1.0 * q.tlen, d->conflict_min_score, false);
            q.min_raw_middle = smallest_raw(1.0 * q.tlen, d->middle_min_score, false);
            if (ragged) {                                             // per barcode: its length and the thresholds that go with it
                q.len_off = (int32_t)hk->ids.size();
                for (int b = 0; b < q.n; ++b) {
                    hk->ids.push_back(bs.lengths[b]);
                    hk->ids.push_back(smallest_raw(1.0 * bs.lengths[b], d->min_quality, false));
                    hk->ids.push_back(smallest_raw(1.0 * bs.lengths[b], d->conflict_min_score, false));
                }
            }
            q.width = barcode_width_class(q.tlen);
            // simple mode on the packed end-tracking kernels (kernels_simple.inc): a list of ONE length that has a simple
            // width class, windows of at most 150 rows, a barcode matrix the binary16 lanes hold; its tables at that width
            if (simple && !ragged && d->max_align_length <= 150 && bf16ok && simple_width_class(q.tlen)) {
                const int sw = simple_width_class(q.tlen);
                const size_t off = hk->tables.size();
                hk->tables.resize(off + (size_t)q.n * sw);
                uint32_t sp = sp_barcode;
                bool ok = true;
                for (int b = 0; b < q.n && ok; ++b)
                    ok = build_fast_tables(k.bmat, &hk->codes[q.tgt_off + (size_t)b * q.tlen], q.tlen, gb,
                                           &hk->tables[off + (size_t)b * sw], &sp, sw, true);
                if (ok) { sp_barcode = sp; q.tbl_off = (int32_t)off; q.width = sw; hk->simple_packed = 1; }
                else hk->tables.resize(off);
            }
            if (fast) {
                size_t off = hk->tables.size();
                hk->tables.resize(off + (size_t)q.n * q.width);
                uint32_t sp = sp_barcode;
                bool ok = q.width != 0;
                for (int b = 0; b < q.n && ok; ++b)
                    ok = build_fast_tables(k.bmat, &hk->codes[q.tgt_off + (size_t)b * q.tlen], q.tlen, gb,
                                           &hk->tables[off + (size_t)b * q.width], &sp, q.width, bf16ok);
                if (ok) { sp_barcode = sp; q.tbl_off = (int32_t)off; }
                else { hk->tables.resize(off); fast = false; }
            }
        }
        if (p.sets[0].n == 0 || (d->mode == QCAT_MODE_DUAL && p.sets[1].n == 0))
            return fail(QCAT_ERR_ARG, "template " + std::to_string(t) +
                        " lacks a barcode set the scanner iterates over (the reference raises TypeError)");
    }
    // 16-bit headroom of the biased DP (H' = H + g(i+j) <= max_w*min(L,M) + g(L+M))
    if (fast) {
        int maxw = 0;
        for (int i = 0; i < 49; ++i) { if (k.amat[i] > maxw) maxw = k.amat[i]; }
        if ((int64_t)maxw * MAX_TLEN + (int64_t)ga * (MAX_WIN + MAX_TLEN) > 60000) fast = false;
        if (ga < 1) fast = false;     // g = 0 would make padding rows free
    }
    {   // bit-sliced barcode kernels: match +1, mismatch -1 between A,T,G,C (windows with any other letter stay off them)
        bool ok = true;
        for (int t = 0; t < 4; ++t)
            for (int qc = 0; qc < 4; ++qc) ok = ok && k.bmat[t * 7 + qc] == (t == qc ? 1 : -1);
        k.bs_ok = (ok && fast) ? 1 : 0;
    }
    k.fast_ok = fast ? 1 : 0;
    k.barcode_f16 = (fast && bf16ok) ? 1 : 0;
    k.special_adapter = sp_adapter == 0xFFFFFFFFu ? 0 : sp_adapter;
    k.special_barcode = sp_barcode == 0xFFFFFFFFu ? 0 : sp_barcode;
    // static adapter kernels (binary16 lanes): every value of the biased DP must stay an exact integer
    {
        int maxw = 0;
        for (int x = 0; x < 5; ++x) {
            uint32_t lo = 0, hi = 0;
            for (int q = 0; q < 8; ++q) {
                const int v = biased_w(k.amat, x, q, ga);
                if (v > maxw) maxw = v;
                const uint16_t b = f16_bits(v);
                k.adapter_w16[x * 8 + q] = b;
                if (q < 4) { lo |= (uint32_t)(b & 0xFF) << (8 * q); hi |= (uint32_t)(b >> 8) << (8 * q); }
            }
            k.adapter_pool_lo[x] = lo; k.adapter_pool_hi[x] = hi;
        }
        const int64_t top = (int64_t)maxw * MAX_TLEN + (int64_t)ga * (MAX_WIN + MAX_TLEN);
        k.adapter_f16 = (fast && top <= 2047) ? 1 : 0;
        k.adapter_f16_headroom = k.adapter_f16 ? (int32_t)(2047 - top) : -1;
    }
    {   // bit-sliced adapter kernels (abs_core.h): the difference form is built on W + 2g in {9, 2, 3} and g = 2
        bool ok = k.adapter_f16 && d->gap_open == 2 && d->gap_extend == 2 && k.max_align >= 8 && k.max_align <= 150;
        for (int t = 0; t < 4 && ok; ++t)
            for (int qc = 0; qc < 4; ++qc) ok = ok && k.amat[t * 7 + qc] == (t == qc ? 5 : -2);
        for (int qc = 0; qc < 4 && ok; ++qc) ok = ok && k.amat[QCAT_CODE_N * 7 + qc] == -1;
        for (int t = 0; t < k.nt && ok; ++t)
            for (int j = 0; j < k.tpl[t].len; ++j) ok = ok && hk->codes[k.tpl[t].code_off + j] <= QCAT_CODE_N;
        k.abs_ok = ok ? 1 : 0;
    }
    for (int x = 0; x < 4; ++x) {
        uint32_t w = 0;
        for (int q = 0; q < 4; ++q) {
            int v = biased_w(k.bmat, x, q, gb);
            if (k.barcode_f16) v = f16_high_byte(v);
            w |= (uint32_t)(v & 0xFF) << (8 * q);
        }
        k.letter_tbl_barcode[x] = w;
    }
    if (hk->codes.empty()) hk->codes.push_back(0);
    if (hk->ids.empty()) hk->ids.push_back(0);
    if (hk->tables.empty()) hk->tables.push_back(0);
    return 0;
}

}  // namespace qk
