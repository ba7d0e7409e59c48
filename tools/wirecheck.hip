// wirecheck.hip — TEST INFRASTRUCTURE. Exposes the device wire decoder
// (narwhal_amd/csrc/nw_wiredec.hpp, compiled as host code) for one frame through a C ABI, so
// tests/test_wire_device_cpu.py can compare the exact scan and emit text the kernels of
// nw_wire.hip run against the Python restatement of the wire format, without a GPU. The
// emit is cooperative: every lane index of the group runs in a loop. wc_canon / wc_emit_canon
// (tests/test_wire_canon_cpu.py) do the same for the canonicalisation of non-canonical
// frames: each phase for every lane index, one phase after the other. wc_place / wc_emit_rec
// (tests/test_wire_place_cpu.py): the host's placement (nw_wireplace.hpp) and the emit over
// the caller's records, forged ones included.
#include <string.h>

#include <algorithm>
#include <vector>

#include "../narwhal_amd/csrc/nw_wireplace.hpp"
#include "wire_single.hpp"

using namespace nw::wd;

// The frame at byte offset `misalign` (0..3) of a word buffer, as the kernels see a frame
// that starts anywhere in the call's byte stream. The bytes around it are 0xA5: nothing
// outside the frame may reach a result.
static std::vector<uint32_t> in_words(const uint8_t* frame, uint64_t len, uint32_t misalign) {
  std::vector<uint32_t> w((misalign + len + 3) / 4 + 1, 0xa5a5a5a5u);
  if (len) memcpy(reinterpret_cast<uint8_t*>(w.data()) + misalign, frame, len);
  return w;
}

// Emits the placed frame with record r (c: its canonicalisation, or null for the plain
// instance) over the buffers of wc_emit, and returns what wc_emit returns.
static long emit_one(const uint32_t* w, uint32_t misalign, uint64_t len, uint32_t group,
                     const rec_t& r, const wire_canon_t* c, uint8_t* hb, uint64_t hb_cap,
                     uint8_t* id32, uint8_t* sig64, uint8_t* vpk, uint8_t* vsig, uint32_t vcap,
                     uint32_t* pc_out, uint64_t* off3_out, uint8_t* vote168) {
  wire_single_t s(r.kind, hb, hb_cap, id32, sig64, vpk, vsig, vcap, vote168, vote168 + 32,
                  vote168 + 40, vote168 + 72, vote168 + 104);
  if (c) s.emit<true>(w, misalign, len, r, &c->c, c->order.data(), c->order.size(), group);
  else s.emit<false>(w, misalign, len, r, nullptr, nullptr, 0, group);
  if (r.kind == 1) return 0;
  *pc_out = s.pc;
  off3_out[0] = s.ho[0];
  off3_out[1] = s.ho[1];
  off3_out[2] = r.kind == 2 ? s.vo[1] : 0;
  return (long)(c ? header_len(c->c.np_u, c->c.nq_u) : header_len(r.np, r.nq));
}

extern "C" {

// rec8: kind, canonical, np, nq, nv, alen, vlen, 0 (wd::rec_t). Returns the kind.
int wc_scan(const uint8_t* frame, uint64_t len, uint32_t misalign, uint32_t* rec8) {
  misalign &= 3;
  const std::vector<uint32_t> w = in_words(frame, len, misalign);
  const rec_t r = scan(w.data(), misalign, len);
  memcpy(rec8, &r, sizeof r);
  return r.kind;
}

// wc_emit with the caller's record r (as wc_scan writes it, or forged: a record that does
// not fit the frame must write nothing) in place of the scan and of the buffer size checks.
// can != null: the instance that serves canonicalised frames, with the caller's canon_t and
// the frame's own order list. What is not written keeps the caller's bytes.
long wc_emit_rec(const uint8_t* frame, uint64_t len, uint32_t misalign, uint32_t group,
                 const rec_t* r, const canon_t* can, uint8_t* hb, uint64_t hb_cap, uint8_t* id32,
                 uint8_t* sig64, uint8_t* vpk, uint8_t* vsig, uint32_t vcap, uint32_t* pc_out,
                 uint64_t* off3_out, uint8_t* vote168) {
  misalign &= 3;
  if (group == 0 || (r->kind != 0 && r->kind != 1 && r->kind != 2)) return -1;
  const std::vector<uint32_t> w = in_words(frame, len, misalign);
  const rec_t none{-1, 0, 0, 0, 0, 0, 0, 0};   // (can = null: nothing to canonicalise)
  wire_canon_t c(w.data(), misalign, len, can ? scan(w.data(), misalign, len) : none, 64);
  if (can) c.c = *can;
  return emit_one(w.data(), misalign, len, group, *r, can ? &c : nullptr, hb, hb_cap, id32, sig64,
                  vpk, vsig, vcap, pc_out, off3_out, vote168);
}

// Scans and emits one frame with a group of `group` lanes. Header / Certificate: hb (hb_cap
// bytes), id32, sig64, vpk / vsig (vcap votes); returns the header byte count. Vote: vote168
// = id 32 | round 8 | origin 32 | author 32 | signature 64; returns 0. -1: the frame has
// nothing to emit (does not decode, non-canonical, a request) or the buffers are too small.
long wc_emit(const uint8_t* frame, uint64_t len, uint32_t misalign, uint32_t group, uint8_t* hb,
             uint64_t hb_cap, uint8_t* id32, uint8_t* sig64, uint8_t* vpk, uint8_t* vsig,
             uint32_t vcap, uint32_t* pc_out, uint64_t* off3_out, uint8_t* vote168) {
  misalign &= 3;
  const std::vector<uint32_t> w = in_words(frame, len, misalign);
  const rec_t r = scan(w.data(), misalign, len);
  if (r.kind != 1 && (!r.canonical || header_len(r.np, r.nq) > hb_cap || r.nv > vcap)) return -1;
  return wc_emit_rec(frame, len, misalign, group, &r, nullptr, hb, hb_cap, id32, sig64, vpk, vsig, vcap,
                     pc_out, off3_out, vote168);
}

// Scans one frame and canonicalises it with `lanes` lanes. Returns the state (kCanon*: 0 not
// applicable, 1 canonicalised, 2 over the bound) or -1 if order_cap is too small. For state
// 1: *np_u / *nq_u = the kept counts, order[0 .. np_u) = the wire index of each kept payload
// entry in key order, order[np_u .. np_u + nq_u) likewise for the parents. *touched = the
// number of scratch words written (any state): exactly np_u + nq_u, or 0.
int wc_canon(const uint8_t* frame, uint64_t len, uint32_t misalign, uint32_t lanes, uint32_t* np_u,
             uint32_t* nq_u, uint32_t* order, uint32_t order_cap, uint32_t* touched) {
  misalign &= 3;
  if (lanes == 0) return -1;
  const std::vector<uint32_t> w = in_words(frame, len, misalign);
  const rec_t r = scan(w.data(), misalign, len);
  const wire_canon_t c(w.data(), misalign, len, r, lanes);
  uint32_t t = 0;
  for (uint32_t x : c.order) t += x != 0xdeadbeefu;
  *touched = t;
  if (c.c.state != kCanonDone) return (int)c.c.state;
  if ((uint64_t)c.c.np_u + c.c.nq_u > order_cap) return -1;
  *np_u = c.c.np_u;
  *nq_u = c.c.nq_u;
  for (uint32_t i = 0; i < c.c.np_u; ++i) order[i] = c.order[c.list + i];
  for (uint32_t i = 0; i < c.c.nq_u; ++i) order[c.c.np_u + i] = c.order[c.list + r.np + i];
  return (int)kCanonDone;
}

// wc_emit for a non-canonical Header / Certificate frame: scan, canonicalise with `lanes`
// lanes, emit through the order list with a group of `group` lanes. Returns the header byte
// count; -1: nothing to emit (the frame does not decode, is canonical, is no Header /
// Certificate, is over the bound) or the buffers are too small.
long wc_emit_canon(const uint8_t* frame, uint64_t len, uint32_t misalign, uint32_t group,
                   uint32_t lanes, uint8_t* hb, uint64_t hb_cap, uint8_t* id32, uint8_t* sig64,
                   uint8_t* vpk, uint8_t* vsig, uint32_t vcap, uint32_t* pc_out,
                   uint64_t* off3_out) {
  misalign &= 3;
  if (group == 0 || lanes == 0) return -1;
  const std::vector<uint32_t> w = in_words(frame, len, misalign);
  const rec_t r = scan(w.data(), misalign, len);
  const wire_canon_t c(w.data(), misalign, len, r, lanes);
  if (c.c.state != kCanonDone) return -1;
  if (header_len(c.c.np_u, c.c.nq_u) > hb_cap || r.nv > vcap) return -1;
  uint8_t no_vote[168];   // (a Header / Certificate: not written)
  return emit_one(w.data(), misalign, len, group, r, &c, hb, hb_cap, id32, sig64, vpk, vsig, vcap,
                  pc_out, off3_out, no_vote);
}

// The host's placement (nw_wireplace.hpp) of n frames (fo: their n + 1 offsets) by the
// caller's records (cans: null = canonicalisation off). cvo (n + 1) / host (n): the vote
// offsets and the host-frame list, their lengths in counts2. Returns the error string, or null.
const char* wc_place(const rec_t* recs, const canon_t* cans, const uint64_t* fo, uint64_t n,
                     uint64_t total, uint64_t vbound, dst_t* dst, place_t* totals, uint64_t* cvo,
                     uint64_t* host, uint64_t* counts2, int32_t* kind, int32_t* status,
                     uint64_t* index) {
  std::vector<uint64_t> cv, hf;
  const char* bad =
      place(recs, cans, fo, n, total, vbound, dst, totals, &cv, &hf, kind, status, index);
  std::copy(cv.begin(), cv.end(), cvo);
  std::copy(hf.begin(), hf.end(), host);
  counts2[0] = cv.size();
  counts2[1] = hf.size();
  return bad;
}

}  // extern "C"
