// text_out.h -- what the text products of a resident batch share on the host (host only, like batch.h): the finished text of a
// call and a device table kept beside its host copy.  The demultiplexed text (fqtext_host.inc), the TSV rows (tsvtext_host.inc)
// and the annotated stream (textstream_host.inc) hold these as members of their scratch (batch.h); the functions are in
// text_out_host.inc.  Included by batch.h.
#pragma once
#include <cstdint>
#include <vector>

#include "dev_buf.h"

// the text a call left on its context: `buf` is slack, text, slack like a batch's planes (text_out_ptr), `first` the first byte
// of every read's part of it with the total behind (n_reads + 1 entries).  A call drops `valid` before it works and sets it in
// text_out_finish: a failed call leaves no text behind.
struct TextOut {
    qk::DevBuf<uint8_t> buf;
    qk::DevBuf<uint64_t> first;
    uint64_t total = 0;
    uint32_t n_reads = 0;
    bool valid = false;
};

// a table on the device and the host copy it was uploaded from.  Invariant: `host` is empty or holds, byte for byte, what was
// written to `dev` -- it never vouches for device memory that nobody wrote, on any early return.  So a call goes in two steps
// around the grow chain that may move `dev` (grow(t.dev, want.size()) is a link of it):
//   stale(want)           in front: true when `want` must go up -- no buffer yet, one too small (it will move), other bytes --, and
//                         then `host` is dropped at once, before anything can fail
//   mirror_upload(...)    behind (text_out_host.inc): `want` becomes `host` once the copy is queued -- `host` is what the copy
//                         reads, so it lives on the context -- and `host` is dropped again if the copy fails
struct MirroredTable {
    qk::DevBuf<uint8_t> dev;
    std::vector<uint8_t> host;
    bool stale(const std::vector<uint8_t>& want) {
        const bool fresh = !dev.get() || dev.cap() < want.size() || want != host;
        if (fresh) host.clear();
        return fresh;
    }
};
