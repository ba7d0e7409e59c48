// wire_single.hpp — TEST INFRASTRUCTURE (tools/wirecheck.hip, tools/wire_canon_san.cpp): one
// frame through the decoder's cooperative steps as the kernels run them, every lane in a loop.
#pragma once
#include <vector>

#include "../narwhal_amd/csrc/nw_wiredec.hpp"

// The wd::out_t of one frame emitted alone, at slot 0 with nothing before it, over the
// caller's buffers. kind 1: the Vote rows v_* (32, 8, 32, 32, 64 bytes). Kind 0 / 2: hb
// (hb_cap bytes), id (32), sig (64), vpk / vsig (32 / 64 bytes per vote, vcap votes).
struct wire_single_t {
  nw::wd::out_t o{};   // (points into this object: not to be copied)
  uint64_t ho[2] = {~0ull, ~0ull}, vo[2] = {~0ull, ~0ull};
  uint32_t pc = ~0u;
  wire_single_t(int kind, void* hb, uint64_t hb_cap, void* id, void* sig, void* vpk, void* vsig,
                uint32_t vcap, void* v_ids, void* v_rounds, void* v_origins, void* v_authors,
                void* v_sigs) {
    auto u32 = [](void* p) { return static_cast<uint32_t*>(p); };
    const int k = kind == 2 ? 1 : 0;
    o.hb[k] = static_cast<uint8_t*>(hb); o.hb_len[k] = hb_cap; o.ho[k] = ho; o.pc[k] = &pc;
    o.ids[k] = u32(id); o.sigs[k] = u32(sig); o.nitems[k] = kind != 1;
    o.vo = vo; o.vpk = u32(vpk); o.vsig = u32(vsig); o.nvotes = vcap;
    o.v_ids = u32(v_ids); o.v_rounds = static_cast<uint64_t*>(v_rounds); o.nvmsg = kind == 1;
    o.v_origins = u32(v_origins); o.v_authors = u32(v_authors); o.v_sigs = u32(v_sigs);
  }
  template <bool kCanon>   // c, order, order_cap: only for kCanon
  void emit(const uint32_t* w, uint64_t off, uint64_t len, const nw::wd::rec_t& r,
            const nw::wd::canon_t* c, const uint32_t* order, uint64_t order_cap, uint32_t group) {
    for (uint32_t l = 0; l < group; ++l)
      nw::wd::emit_lane<kCanon>(w, off, len, r, c, order, order_cap, {0, 0, 0}, o, l, group);
  }
};

// The canonicalisation of the frame at byte offset off of w as k_wire_canon runs it: every
// phase for every lane index, one phase after the other (the loop boundary is the kernel's
// barrier). order: the scratch of a byte stream that ends with this frame; list: its list.
struct wire_canon_t {
  nw::wd::canon_t c{0, 0, nw::wd::kCanonNone, 0};
  std::vector<uint32_t> order;
  uint64_t list = 0;
  wire_canon_t(const uint32_t* w, uint64_t off, uint64_t len, const nw::wd::rec_t& r,
               uint32_t lanes) : order(nw::wd::canon_list_words(off + len), 0xdeadbeefu) {
    using namespace nw::wd;
    canon_job_t jb;
    c.state = canon_begin(w, off, len, r, order.size(), &jb);
    if (c.state != kCanonDone) return;
    list = jb.list;
    std::vector<uint32_t> kept(r.np + r.nq, 0xa5a5a5a5u), keys(8 * kept.size(), 0xa5a5a5a5u);
    for (uint32_t l = 0; l < lanes; ++l) canon_stage(l, lanes, jb, keys.data());
    for (uint32_t l = 0; l < lanes; ++l) canon_mark(l, lanes, jb, keys.data(), kept.data());
    for (uint32_t l = 0; l < lanes; ++l)
      canon_rank(l, lanes, jb, keys.data(), kept.data(), order.data(), &c);
  }
};
