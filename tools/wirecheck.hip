// wirecheck.hip — TEST INFRASTRUCTURE. Exposes the device wire decoder
// (narwhal_amd/csrc/nw_wiredec.hpp, compiled as host code) for one frame through a C ABI, so
// tests/test_wire_device_cpu.py can compare the exact scan and emit text the kernels of
// nw_wire.hip run against the Python restatement of the wire format, without a GPU. The
// emit is cooperative: every lane index of the group runs in a loop.
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
