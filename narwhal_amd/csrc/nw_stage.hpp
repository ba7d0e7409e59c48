// nw_stage.hpp — the staged layout of the message jobs' inputs (host only, no HIP calls).
//
// Every path that verifies primary messages lays the same groups of arrays into 256-byte
// aligned sections: the committee, then the header stream, the certificates' votes, or the
// Vote messages. Each array's width and position is stated here and nowhere else. Per group:
//   plan_*(Packer&, counts) -> the sections in buffer order (optional arrays by argument);
//   fill_*(host base, sections, the caller's arrays): the copies;
//   view_*(any base, sections) -> typed pointers: the pinned buffer, its device address, a
//                                 device copy of it, or a device-only region nothing filled.
// A section not planned stays unstaged: filled with nothing, viewed as a null pointer.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "narwhal_amd.h"

namespace nw {
namespace stage {

inline size_t a256(size_t x) { return (x + 255) & ~(size_t)255; }

struct Sec {
  size_t off = ~(size_t)0, bytes = 0;
  bool staged() const { return off != ~(size_t)0; }
};

// 256-byte aligned sections of a job's staging buffers (pinned and device share one layout);
// an empty section still takes one (distinct offsets).
struct Packer {
  size_t off = 0;
  size_t add(size_t bytes) {
    const size_t o = off;
    off += a256(bytes ? bytes : 1);
    return o;
  }
  Sec sec(size_t bytes) { return Sec{add(bytes), bytes}; }
};

inline void put(char* base, const Sec& s, const void* src) {
  if (s.staged() && s.bytes) memcpy(base + s.off, src, s.bytes);
}
template <class T>
inline const T* at(const char* base, const Sec& s) {
  return s.staged() ? reinterpret_cast<const T*>(base + s.off) : nullptr;
}

// ---- the committee ----------------------------------------------------------------------
struct CommitteeOffs {
  Sec pks, stakes, wo, wi;
};
inline CommitteeOffs plan_committee(Packer& P, const nw_committee* com) {
  const size_t na = com->nauth, nwk = na ? com->worker_offsets[na] : 0;
  CommitteeOffs o;
  o.pks = P.sec(32 * na);
  o.stakes = P.sec(4 * na);
  o.wo = P.sec(8 * (na + 1));
  o.wi = P.sec(4 * nwk);
  return o;
}
inline void fill_committee(char* h, const CommitteeOffs& o, const nw_committee* com) {
  put(h, o.pks, com->pks);
  put(h, o.stakes, com->stakes);
  put(h, o.wo, com->worker_offsets);
  put(h, o.wi, com->worker_ids);
}
inline nw_committee view_committee(const char* base, const CommitteeOffs& o, size_t na) {
  nw_committee d;
  d.nauth = na;
  d.pks = at<uint8_t>(base, o.pks);
  d.stakes = at<uint32_t>(base, o.stakes);
  d.worker_offsets = at<uint64_t>(base, o.wo);
  d.worker_ids = at<uint32_t>(base, o.wi);
  return d;
}

// ---- the header stream: n headers, hlen header bytes -------------------------------------
struct HeaderOffs {
  Sec hb, ho, pc, id, hs;
};
inline HeaderOffs plan_headers(Packer& P, size_t n, size_t hlen) {
  HeaderOffs o;
  o.hb = P.sec(hlen);
  o.ho = P.sec(8 * (n + 1));
  o.pc = P.sec(4 * n);
  o.id = P.sec(32 * n);
  o.hs = P.sec(64 * n);
  return o;
}
// cs->header_offsets may start anywhere (a fan-out part's do): the staged ones start at 0 and
// the staged bytes are those from header_offsets[0] on.
inline void fill_headers(char* h, const HeaderOffs& o, const nw_certificates* cs) {
  const uint64_t hb0 = cs->header_offsets[0];
  put(h, o.hb, cs->header_bytes + hb0);
  uint64_t* ho = reinterpret_cast<uint64_t*>(h + o.ho.off);
  for (size_t i = 0; i <= cs->n; ++i) ho[i] = cs->header_offsets[i] - hb0;
  put(h, o.pc, cs->payload_counts);
  put(h, o.id, cs->ids);
  put(h, o.hs, cs->header_sigs);
}
// (the vote fields stay null: view_cert_votes)
inline nw_certificates view_headers(const char* base, const HeaderOffs& o, size_t n, size_t hlen) {
  nw_certificates d{};
  d.n = n;
  d.header_bytes = at<uint8_t>(base, o.hb);
  d.header_offsets = at<uint64_t>(base, o.ho);
  d.payload_counts = at<uint32_t>(base, o.pc);
  d.ids = at<uint8_t>(base, o.id);
  d.header_sigs = at<uint8_t>(base, o.hs);
  d.header_bytes_len = hlen;
  return d;
}

// ---- the certificates' votes: nv votes of n certificates ---------------------------------
// with_offsets: the n + 1 vote offsets (the small-job launch reads its slots instead);
// with_z16: injected batch coefficients.
struct CertVoteOffs {
  Sec vo, vp, vs, z;
};
inline CertVoteOffs plan_cert_votes(Packer& P, size_t n, size_t nv, bool with_offsets,
                                    bool with_z16) {
  CertVoteOffs o;
  if (with_offsets) o.vo = P.sec(8 * (n + 1));
  o.vp = P.sec(32 * nv);
  o.vs = P.sec(64 * nv);
  if (with_z16) o.z = P.sec(16 * nv);
  return o;
}
inline void fill_cert_votes(char* h, const CertVoteOffs& o, const nw_certificates* cs,
                            const uint8_t* z16) {
  put(h, o.vo, cs->vote_offsets);
  put(h, o.vp, cs->vote_pks);
  put(h, o.vs, cs->vote_sigs);
  put(h, o.z, z16);
}
// Adds the votes to a view_headers result; returns the staged z16 (null: none).
inline const uint8_t* view_cert_votes(const char* base, const CertVoteOffs& o, size_t nv,
                                      nw_certificates* d) {
  d->vote_offsets = at<uint64_t>(base, o.vo);
  d->vote_pks = at<uint8_t>(base, o.vp);
  d->vote_sigs = at<uint8_t>(base, o.vs);
  d->nvotes = o.vp.staged() ? nv : 0;
  return at<uint8_t>(base, o.z);
}

// ---- Vote messages: the caller's arrays, and a view of the staged ones -------------------
struct VoteMsgs {
  const uint8_t* ids;
  const uint64_t* rounds;
  const uint8_t *origins, *authors, *sigs;
  size_t n;
};
struct VoteMsgOffs {
  Sec id, rd, org, au, sg;
};
inline VoteMsgOffs plan_vote_msgs(Packer& P, size_t n) {
  VoteMsgOffs o;
  o.id = P.sec(32 * n);
  o.rd = P.sec(8 * n);
  o.org = P.sec(32 * n);
  o.au = P.sec(32 * n);
  o.sg = P.sec(64 * n);
  return o;
}
inline void fill_vote_msgs(char* h, const VoteMsgOffs& o, const VoteMsgs& v) {
  put(h, o.id, v.ids);
  put(h, o.rd, v.rounds);
  put(h, o.org, v.origins);
  put(h, o.au, v.authors);
  put(h, o.sg, v.sigs);
}
inline VoteMsgs view_vote_msgs(const char* base, const VoteMsgOffs& o, size_t n) {
  return VoteMsgs{at<uint8_t>(base, o.id),  at<uint64_t>(base, o.rd), at<uint8_t>(base, o.org),
                  at<uint8_t>(base, o.au), at<uint8_t>(base, o.sg),  n};
}

// ---- per-item messages of any length (the SHA-512, strict and verify_batch jobs) -----------
// Message i is lengths[i] bytes at data + offsets[i]: anywhere in `data`, in any order,
// overlapping or not. The jobs stage them packed in item order: offs_out[i] = the bytes before
// message i, and dst gets the bytes (runs that are contiguous in `data` in one copy). data may
// be null when every message is empty. messages_bytes: what dst must hold.
inline uint64_t messages_bytes(const uint64_t* lengths, size_t n) {
  uint64_t total = 0;
  for (size_t i = 0; i < n; ++i) total += lengths[i];
  return total;
}
inline void pack_messages(char* dst, uint64_t* offs_out, const uint8_t* data,
                          const uint64_t* offsets, const uint64_t* lengths, size_t n) {
  uint64_t pos = 0;
  for (size_t i = 0; i < n; ++i) {
    offs_out[i] = pos;
    pos += lengths[i];
  }
  size_t i = 0;
  while (i < n) {
    size_t k = i + 1;
    while (k < n && offsets[k] == offsets[k - 1] + lengths[k - 1]) ++k;
    const uint64_t bytes = offs_out[k - 1] + lengths[k - 1] - offs_out[i];
    if (bytes) memcpy(dst + offs_out[i], data + offsets[i], bytes);
    i = k;
  }
}

// ---- a verify_batch job (nw_jobs.cpp submit_batch) ----------------------------------------
// The inputs are [0, st): the batch digests, or for a call over per-vote messages
// (msg_bytes != kNoMsgs) the packed bytes with their offsets and lengths; then the vote offsets,
// keys, signatures and (z16) coefficients. The outputs are [st, ws): statuses, failing indices,
// a digest call's done word (NW_BATCH_SPIN; a lone fused batch's input-gate flags sit at `st` of
// its device-memory buffer instead) and, with `signers`, the comb phase's six counters. Device
// only from `ws` on: the batch workspace (ws_bytes), a message call's k plane (32 bytes per
// vote), the comb phase's scratch (sg_bytes). A section a call does not have is empty.
constexpr size_t kNoMsgs = ~(size_t)0;
struct BatchOffs {
  size_t data, mo, ml, d, off, pk, sig, z, st, fi, dn, ct, ws, kp, sg, end;
};
inline BatchOffs plan_batch(size_t nbatches, size_t nitems, size_t msg_bytes, bool z16,
                            bool signers, size_t ws_bytes, size_t sg_bytes) {
  const bool msgs = msg_bytes != kNoMsgs;
  const size_t m = nitems ? nitems : 1;
  size_t o = 0;
  const auto sec = [&o](bool present, size_t bytes) {
    const size_t at = o;
    if (present) o += a256(bytes);
    return at;
  };
  BatchOffs p;
  p.data = sec(msgs, msg_bytes ? msg_bytes : 1);
  p.mo = sec(msgs, 8 * m);
  p.ml = sec(msgs, 8 * m);
  p.d = sec(!msgs, 32 * nbatches);
  p.off = sec(true, 8 * (nbatches + 1));
  p.pk = sec(true, 32 * m);
  p.sig = sec(true, 64 * m);
  p.z = sec(z16, 16 * m);
  p.st = sec(true, 4 * nbatches);
  p.fi = sec(true, 8 * nbatches);
  p.dn = sec(!msgs, 256);
  p.ct = sec(signers, 256);
  p.ws = sec(true, ws_bytes);
  p.kp = sec(msgs, 32 * m);
  p.sg = sec(signers, sg_bytes);
  p.end = o;
  return p;
}

}  // namespace stage
}  // namespace nw
