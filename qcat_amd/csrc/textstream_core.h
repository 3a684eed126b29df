// textstream_core.h -- the arithmetic of the driver's annotated single stream in device memory (kernels_textstream.inc,
// textstream_host.inc), as pure functions that compile for host and device: the tag plane's layout, the segment table of one
// output record, the decoding of a two-plane source position, and the output's upper bound.  tests/textstream_check.cpp runs
// the copy's chunk and lane schedule through these and partition_core.h on the host.
//
// Vocabulary.  The STREAM is what the driver writes without -b and without --tsv (qcat/cli.py:345-358; FqWriter::write_range's
// !to_dir branch in fastq_host.inc): every kept read in read order,
//   sigil title sep "barcode=" id '\n' seq[a:b] "\n+\n" qual[a:b] '\n'          FASTQ
//   sigil title sep "barcode=" id '\n' seq[a:b] '\n'                            FASTA
// sigil = the byte in front of the stored title, sep = one blank when the stored title holds a blank and two when it holds none
// (name + " " + comment + " barcode="), id = str(Barcode.id) of a called read (dual mode: id "/" id2) and "none" of any other.
// A record is ANNOT_SEGS SEGMENTS, each a length and a source position.  The sources lie in two PLANES: the text plane of the
// batch, and the TAG plane -- the blob of the TSV tables (qtsv::tables_build: its id slots hold the id texts) with
// ANNOT_CONST_BYTES of constants behind it, and the copy's slack on both sides like a batch's planes.  A source position in the
// tag plane carries ANNOT_TAG.  The copy is the partition's (qpart::gather_vectors<1>), its load decoding the plane.
#pragma once
#include <stdint.h>

#include "fqtext_core.h"
#include "partition_core.h"
#include "tsvtext_core.h"

namespace qann {

constexpr uint32_t ANNOT_SEGS = 10;    // sigil + title, sep + "barcode=", id, "/", id2, '\n', seq, "\n+\n", qual, '\n'
// Bit 62, not 63: the gather computes SIGNED aligned offsets from -16 on (a slice that starts inside the first vector of its
// plane), so a text-plane offset may be negative; with bit 62 a tag-plane offset stays positive and far from every text offset.
constexpr uint64_t ANNOT_TAG = 1ull << 62;
constexpr uint32_t ANNOT_CONST_BYTES = 32;
// the constants behind the blob: "  barcode=" at 0 (a sep of one blank starts at 1), "none" at 10, "/" at 14, "\n" at 15,
// "\n+\n" at 16, "\n" at 19
constexpr uint32_t AN_C_SEP2 = 0, AN_C_SEP1 = 1, AN_C_SEP2_LEN = 10, AN_C_NONE = 10, AN_C_NONE_LEN = 4, AN_C_SLASH = 14, AN_C_NL = 15,
                   AN_C_PLUS = 16, AN_C_LAST_NL = 19;
QP_HD void annot_constants(uint8_t* c /* ANNOT_CONST_BYTES */) {
    const char s[21] = "  barcode=none/\n\n+\n\n";
    for (uint32_t i = 0; i < ANNOT_CONST_BYTES; ++i) c[i] = i < 20 ? (uint8_t)s[i] : 0;
}
// where the constants lie in the tag plane behind a blob of blob_bytes bytes, and the plane's size (without the slack)
QP_HD uint64_t tag_const_off(uint64_t blob_bytes) { return (blob_bytes + 15ull) & ~15ull; }
QP_HD uint64_t tag_plane_bytes(uint64_t blob_bytes) { return tag_const_off(blob_bytes) + ANNOT_CONST_BYTES; }

// ---- a two-plane source: the aligned offset the gather asks for, decoded -----------------------------------------------------------
QP_HD bool src_in_tag(int64_t a) { return a >= (int64_t)(ANNOT_TAG >> 1); }
QP_HD int64_t src_plane_off(int64_t a) { return src_in_tag(a) ? a - (int64_t)ANNOT_TAG : a; }

// ---- one record of the stream: ten (length, source position) pairs; a dropped read: zeros.  T.blob: the tag plane's blob (the
// id slots' length bytes are read), const_off: where the constants lie in the tag plane; [s, s + keep) the kept slice ------------
QP_HD void record_segments(const qtsv::Tables& T, const qfq::Rec& r, bool fasta, uint64_t s, uint64_t keep, bool skipped, int32_t bc,
                           int32_t bc2, int32_t adapter, uint64_t const_off, uint64_t* len, uint64_t* src) {
    for (uint32_t i = 0; i < ANNOT_SEGS; ++i) { len[i] = 0; src[i] = 0; }
    if (skipped) return;
    const uint64_t c = ANNOT_TAG | const_off;
    len[0] = 1 + (uint64_t)r.title_len;           src[0] = r.title_off - 1;
    len[1] = AN_C_SEP2_LEN - (r.title_blank ? 1 : 0); src[1] = c + (r.title_blank ? AN_C_SEP1 : AN_C_SEP2);
    if (qtsv::called(T, bc, bc2, adapter)) {
        const uint32_t t = T.simple ? 0u : (uint32_t)adapter;
        const uint32_t slot = T.ids_off + (T.id_first[t][0] + (uint32_t)bc) * qtsv::TSV_ID_SLOT;
        len[2] = T.blob[slot];                    src[2] = ANNOT_TAG | ((uint64_t)slot + 1u);
        if (T.dual) {
            const uint32_t slot2 = T.ids_off + (T.id_first[t][1] + (uint32_t)bc2) * qtsv::TSV_ID_SLOT;
            len[3] = 1;                           src[3] = c + AN_C_SLASH;
            len[4] = T.blob[slot2];               src[4] = ANNOT_TAG | ((uint64_t)slot2 + 1u);
        }
    } else {
        len[2] = AN_C_NONE_LEN;                   src[2] = c + AN_C_NONE;
    }
    len[5] = 1;                                   src[5] = c + AN_C_NL;
    len[6] = keep;                                src[6] = r.seq_off + s;
    if (!fasta) {
        len[7] = 3;                               src[7] = c + AN_C_PLUS;
        len[8] = keep;                            src[8] = r.qual_off + s;
    }
    len[9] = 1;                                   src[9] = c + AN_C_LAST_NL;
}

// an upper bound of the stream of n reads parsed from n_bytes of text.  A FASTQ record of the text has at least
// 1 + title + 1 + seq + 3 + seq bytes and one of the stream at most 1 + title + 10 + id + 1 + seq + 3 + seq + 1; a FASTA record
// at least 1 + title + 1 + seq and at most 1 + title + 10 + id + 1 + seq + 1: 11 + id more either way, id the longest id text
// ("none", or the longest id, "/" and the longest second id in dual mode); the text's last newline may be missing
QP_HD uint64_t id_bound(const qtsv::Tables& T) {
    const uint64_t id = (uint64_t)T.max_id[0] + (T.dual ? 1u + (uint64_t)T.max_id[1] : 0u);
    return id > AN_C_NONE_LEN ? id : AN_C_NONE_LEN;
}
QP_HD uint64_t output_bound(uint64_t n_bytes, uint64_t n, const qtsv::Tables& T) { return n_bytes + n * (11 + id_bound(T)) + 1; }

}  // namespace qann
