// nw_wireplace.hpp — host only: step 3 of nw::rt::wire_verify_device (nw_jobs.cpp), which
// tools/wirecheck.hip also runs without a GPU (wc_place, tests/test_wire_place_cpu.py).
#pragma once
#include <vector>

#include "narwhal_amd.h"
#include "nw_wiredec.hpp"

namespace nw {
namespace wd {

// Headers / certificates, their header bytes, Vote messages, votes, canonicalised frames.
struct place_t { uint64_t cnt[2], hbl[2], nvm, nvotes, ncanon; };

// Places frames [fo[i], fo[i + 1]), i < n, by the records (and, can != null: canonicalisation
// on, the canon_t array) the device wrote, trusting nothing in them: every record is held
// against its own frame's length (header_layout / vote_layout), a canonicalised frame's kept
// counts against the raw ones, the totals against the bounds the buffers were sized with.
// Writes dst[i] (kNoSlot: nothing to emit), *p, cvo (the certificates' vote offsets) and
// appends the host decoder's frames to host_frames; kind_out / status_out / index_out (the
// last may be null) get every other frame's kind and, where no device check follows, verdict.
// Returns null, or a static string naming what is wrong with the first bad record.
inline const char* place(const rec_t* rec, const canon_t* can, const uint64_t* fo, size_t n,
                         uint64_t total, uint64_t vbound, dst_t* dst, place_t* p,
                         std::vector<uint64_t>* cvo, std::vector<uint64_t>* host_frames,
                         int32_t* kind_out, int32_t* status_out, uint64_t* index_out) {
  *p = place_t{};
  cvo->assign(1, 0);
  const char* bad = nullptr;
  for (size_t i = 0; i < n && !bad; ++i) {
    const rec_t& r = rec[i];
    dst[i] = dst_t{0, kNoSlot, 0};
    const bool noncanon = (r.kind == 0 || r.kind == 2) && !r.canonical;
    if (r.kind == kOverCap || (noncanon && (!can || can[i].state == kCanonOver))) {
      host_frames->push_back(i);
      continue;
    }
    kind_out[i] = r.kind;
    status_out[i] = r.kind < 0 ? NW_DAG_SERIALIZATION : 0;
    if (index_out) index_out[i] = 0;
    if (r.kind == -1 || r.kind == NW_MSG_CERTIFICATES_REQUEST) continue;
    if (r.kind == NW_MSG_VOTE) {
      if (!vote_layout(fo[i], fo[i + 1] - fo[i], r).ok) bad = "vote record";
      dst[i].slot = (uint32_t)p->nvm++;
      continue;
    }
    if (r.kind != NW_MSG_HEADER && r.kind != NW_MSG_CERTIFICATE) return "record kind";
    const int k = r.kind == NW_MSG_CERTIFICATE;
    uint64_t hl = header_len(r.np, r.nq);
    if (noncanon) {   // the kept counts: at most the raw ones, and none only where none was sent
      const canon_t& c = can[i];
      if (c.state != kCanonDone || c.np_u > r.np || c.nq_u > r.nq || (r.np && !c.np_u) ||
          (r.nq && !c.nq_u))
        bad = "canon record";
      hl = header_len(c.np_u, c.nq_u);
      ++p->ncanon;
    }
    if (!header_layout(fo[i], fo[i + 1] - fo[i], r).ok) bad = "header record";
    dst[i] = dst_t{p->hbl[k], (uint32_t)p->cnt[k]++, (uint32_t)p->nvotes};
    p->hbl[k] += hl;
    if (k) {
      p->nvotes += r.nv;
      cvo->push_back(p->nvotes);
    }
  }
  if (!bad && (p->hbl[0] + p->hbl[1] > total || p->nvotes > vbound)) bad = "record totals";
  return bad;
}

}  // namespace wd
}  // namespace nw
