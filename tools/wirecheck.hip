// wirecheck.hip — TEST INFRASTRUCTURE. Exposes the device wire decoder
// (narwhal_amd/csrc/nw_wiredec.hpp, compiled as host code) for one frame through a C ABI, so
// tests/test_wire_device_cpu.py can compare the exact scan and emit text the kernels of
// nw_wire.hip run against the Python restatement of the wire format, without a GPU. The
// emit is cooperative: every lane index of the group runs in a loop. wc_canon / wc_emit_canon
// (tests/test_wire_canon_cpu.py) do the same for the canonicalisation of non-canonical
// frames: each phase for every lane index, one phase after the other.
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../narwhal_amd/csrc/nw_wiredec.hpp"

using namespace nw::wd;

// The frame at byte offset `misalign` (0..3) of a word buffer, as the kernels see a frame
// that starts anywhere in the call's byte stream. The bytes around it are 0xA5: nothing
// outside the frame may reach a result.
static std::vector<uint32_t> place(const uint8_t* frame, uint64_t len, uint32_t misalign) {
  std::vector<uint32_t> w((misalign + len + 3) / 4 + 1, 0xa5a5a5a5u);
  if (len) memcpy(reinterpret_cast<uint8_t*>(w.data()) + misalign, frame, len);
  return w;
}

extern "C" {

// rec8: kind, canonical, np, nq, nv, alen, vlen, 0 (wd::rec_t). Returns the kind.
int wc_scan(const uint8_t* frame, uint64_t len, uint32_t misalign, uint32_t* rec8) {
  misalign &= 3;
  const std::vector<uint32_t> w = place(frame, len, misalign);
  const rec_t r = scan(w.data(), misalign, len);
  memcpy(rec8, &r, sizeof r);
  return r.kind;
}

// Scans and emits one frame with a group of `group` lanes. Header / Certificate: hb (hb_cap
// bytes), id32, sig64, vpk / vsig (vcap votes); returns the header byte count. Vote: vote168
// = id 32 | round 8 | origin 32 | author 32 | signature 64; returns 0. -1: the frame has
// nothing to emit (does not decode, non-canonical, a request) or the buffers are too small.
long wc_emit(const uint8_t* frame, uint64_t len, uint32_t misalign, uint32_t group, uint8_t* hb,
             uint64_t hb_cap, uint8_t* id32, uint8_t* sig64, uint8_t* vpk, uint8_t* vsig,
             uint32_t vcap, uint32_t* pc_out, uint64_t* off3_out, uint8_t* vote168) {
  misalign &= 3;
  if (group == 0) return -1;
  const std::vector<uint32_t> w = place(frame, len, misalign);
  const rec_t r = scan(w.data(), misalign, len);
  if (r.kind != 0 && r.kind != 1 && r.kind != 2) return -1;
  if (r.kind != 1 && !r.canonical) return -1;
  const dst_t d{0, 0, 0};
  uint64_t ho[2] = {~0ull, ~0ull}, vo[2] = {~0ull, ~0ull}, round = 0;
  uint32_t pc = ~0u;
  out_t o{};
  const int k = r.kind == 2 ? 1 : 0;
  if (r.kind == 1) {
    o.v_ids = reinterpret_cast<uint32_t*>(vote168);
    o.v_rounds = &round;
    o.v_origins = reinterpret_cast<uint32_t*>(vote168 + 40);
    o.v_authors = reinterpret_cast<uint32_t*>(vote168 + 72);
    o.v_sigs = reinterpret_cast<uint32_t*>(vote168 + 104);
    o.nvmsg = 1;
  } else {
    if (header_len(r) > hb_cap || r.nv > vcap) return -1;
    o.hb[k] = hb;
    o.hb_len[k] = hb_cap;
    o.ho[k] = ho;
    o.pc[k] = &pc;
    o.ids[k] = reinterpret_cast<uint32_t*>(id32);
    o.sigs[k] = reinterpret_cast<uint32_t*>(sig64);
    o.nitems[k] = 1;
    o.vo = vo;
    o.vpk = reinterpret_cast<uint32_t*>(vpk);
    o.vsig = reinterpret_cast<uint32_t*>(vsig);
    o.nvotes = vcap;
  }
  for (uint32_t lane = 0; lane < group; ++lane)
    emit_lane(w.data(), misalign, len, r, d, o, lane, group);
  if (r.kind == 1) {
    memcpy(vote168 + 32, &round, 8);
    return 0;
  }
  *pc_out = pc;
  off3_out[0] = ho[0];
  off3_out[1] = ho[1];
  off3_out[2] = k ? vo[1] : 0;
  return (long)header_len(r);
}

}  // extern "C"

// The canonicalisation of one placed frame as k_wire_canon runs it: every phase for every
// lane index, one phase after the other (the loop boundary is the kernel's barrier). The
// scratch is sized as the job sizes it, for a byte stream that ends with this frame.
struct canon_run_t {
  canon_t c{0, 0, kCanonNone, 0};
  std::vector<uint32_t> order;
  uint64_t list = 0;
};
static canon_run_t run_canon(const uint32_t* w, uint32_t misalign, uint64_t len, const rec_t& r,
                             uint32_t lanes) {
  canon_run_t out;
  out.order.assign(canon_list_words(misalign + len), 0xdeadbeefu);
  canon_job_t jb;
  out.c.state = canon_begin(w, misalign, len, r, out.order.size(), &jb);
  if (out.c.state != kCanonDone) return out;
  out.list = jb.list;
  std::vector<uint32_t> keys(8 * kCanonMax, 0xa5a5a5a5u), kept(kCanonMax, 0xa5a5a5a5u);
  for (uint32_t l = 0; l < lanes; ++l) canon_stage(l, lanes, jb, keys.data());
  for (uint32_t l = 0; l < lanes; ++l) canon_mark(l, lanes, jb, keys.data(), kept.data());
  for (uint32_t l = 0; l < lanes; ++l)
    canon_rank(l, lanes, jb, keys.data(), kept.data(), out.order.data(), &out.c);
  return out;
}

extern "C" {

// Scans one frame and canonicalises it with `lanes` lanes. Returns the state (kCanon*: 0 not
// applicable, 1 canonicalised, 2 over the bound) or -1 if order_cap is too small. For state
// 1: *np_u / *nq_u = the kept counts, order[0 .. np_u) = the wire index of each kept payload
// entry in key order, order[np_u .. np_u + nq_u) likewise for the parents. *touched = the
// number of scratch words written (any state): exactly np_u + nq_u, or 0.
int wc_canon(const uint8_t* frame, uint64_t len, uint32_t misalign, uint32_t lanes, uint32_t* np_u,
             uint32_t* nq_u, uint32_t* order, uint32_t order_cap, uint32_t* touched) {
  misalign &= 3;
  if (lanes == 0) return -1;
  const std::vector<uint32_t> w = place(frame, len, misalign);
  const rec_t r = scan(w.data(), misalign, len);
  const canon_run_t c = run_canon(w.data(), misalign, len, r, lanes);
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
  const std::vector<uint32_t> w = place(frame, len, misalign);
  const rec_t r = scan(w.data(), misalign, len);
  const canon_run_t c = run_canon(w.data(), misalign, len, r, lanes);
  if (c.c.state != kCanonDone) return -1;
  if (header_len(c.c) > hb_cap || r.nv > vcap) return -1;
  const dst_t d{0, 0, 0};
  uint64_t ho[2] = {~0ull, ~0ull}, vo[2] = {~0ull, ~0ull};
  uint32_t pc = ~0u;
  out_t o{};
  const int k = r.kind == 2 ? 1 : 0;
  o.hb[k] = hb;
  o.hb_len[k] = hb_cap;
  o.ho[k] = ho;
  o.pc[k] = &pc;
  o.ids[k] = reinterpret_cast<uint32_t*>(id32);
  o.sigs[k] = reinterpret_cast<uint32_t*>(sig64);
  o.nitems[k] = 1;
  o.vo = vo;
  o.vpk = reinterpret_cast<uint32_t*>(vpk);
  o.vsig = reinterpret_cast<uint32_t*>(vsig);
  o.nvotes = vcap;
  for (uint32_t lane = 0; lane < group; ++lane)
    emit_lane_canon(w.data(), misalign, len, r, c.c, c.order.data(), c.order.size(), d, o, lane,
                    group);
  *pc_out = pc;
  off3_out[0] = ho[0];
  off3_out[1] = ho[1];
  off3_out[2] = k ? vo[1] : 0;
  return (long)header_len(c.c);
}

}  // extern "C"
