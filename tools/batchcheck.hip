// batchcheck.hip — TEST INFRASTRUCTURE. The host side of a verify_batch call through a C ABI, so
// tests/test_batch_call_cpu.py can run it without a GPU: the refusal rules
// (narwhal_amd/csrc/nw_batch_call.hpp batch_call_check), the batch job's section plan and the
// packing of per-item messages (nw_stage.hpp plan_batch, pack_messages). The stand-alone form
// (`make batchsan`, this file with its main under AddressSanitizer / UBSan) packs into buffers of
// exactly the packed size from sources of exactly their size, so any access past an end is seen.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../narwhal_amd/csrc/nw_batch_call.hpp"
#include "../narwhal_amd/csrc/nw_stage.hpp"

namespace stg = nw::stage;

extern "C" {

// One combination of a call's options: each flag says whether the pointer is there;
// gate_chunk < 0: no gate. Returns batch_call_check's value (0: accepted).
int bc_check(int keys, int skip, uint64_t skip_per_group, double active_frac, int skip_pip,
             int votes, int kplane, int fuse_ctr, long gate_chunk, int done, int gate_ok,
             int outputs_direct, uint64_t nbatches, uint64_t nitems, int digests) {
  static uint32_t word[8];   // what the opaque pointers point at (never read)
  const nw::input_gate_t gate{word, 1u, (uint32_t)(gate_chunk < 0 ? 0 : gate_chunk)};
  nw::batch_call_t c;
  c.digests = digests ? word : nullptr;
  c.nbatches = nbatches;
  c.nitems = nitems;
  c.keys = keys ? reinterpret_cast<const nw::key_tables_t*>(word) : nullptr;
  c.skip_group_ok = skip ? word : nullptr;
  c.skip_per_group = skip_per_group;
  c.active_frac = active_frac;
  c.skip_pip = skip_pip != 0;
  c.votes = votes ? reinterpret_cast<const nw::batch_votes_t*>(word) : nullptr;
  c.kplane = kplane != 0;
  c.fuse_ctr = fuse_ctr ? word : nullptr;
  c.gate = gate_chunk < 0 ? nullptr : &gate;
  c.done = done ? word : nullptr;
  return (int)nw::batch_call_check(c, gate_ok != 0, outputs_direct != 0);
}

// The defaults of a batch_call_t's options, in bc_check's order (skip_per_group, active_frac,
// then the flags keys, skip, skip_pip, votes, kplane, fuse_ctr, gate, done).
void bc_defaults(uint64_t* skip_per_group, double* active_frac, int flags[8]) {
  const nw::batch_call_t c;
  *skip_per_group = c.skip_per_group;
  *active_frac = c.active_frac;
  const bool f[8] = {c.keys != nullptr,  c.skip_group_ok != nullptr, c.skip_pip,
                     c.votes != nullptr, c.kplane,                   c.fuse_ctr != nullptr,
                     c.gate != nullptr,  c.done != nullptr};
  for (int i = 0; i < 8; ++i) flags[i] = f[i];
}

// out: data, mo, ml, d, off, pk, sig, z, st, fi, dn, ct, ws, kp, sg, end. msg_bytes < 0: a
// digest call.
void bc_plan(uint64_t nbatches, uint64_t nitems, long long msg_bytes, int z16, int signers,
             uint64_t ws_bytes, uint64_t sg_bytes, uint64_t out[16]) {
  const stg::BatchOffs p =
      stg::plan_batch(nbatches, nitems, msg_bytes < 0 ? stg::kNoMsgs : (size_t)msg_bytes, z16 != 0,
                      signers != 0, ws_bytes, sg_bytes);
  const size_t v[16] = {p.data, p.mo, p.ml, p.d,  p.off, p.pk, p.sig, p.z,
                        p.st,   p.fi, p.dn, p.ct, p.ws,  p.kp, p.sg,  p.end};
  for (int i = 0; i < 16; ++i) out[i] = v[i];
}

// Packs into a buffer of exactly messages_bytes(lengths, n) and copies it to dst (that many
// bytes); returns the count.
uint64_t bc_pack(uint8_t* dst, uint64_t* offs_out, const uint8_t* data, const uint64_t* offsets,
                 const uint64_t* lengths, uint64_t n) {
  const uint64_t total = stg::messages_bytes(lengths, n);
  char* buf = static_cast<char*>(malloc(total ? total : 1));
  uint64_t* offs = static_cast<uint64_t*>(malloc(n ? 8 * n : 1));
  stg::pack_messages(buf, offs, data, offsets, lengths, n);
  if (total) memcpy(dst, buf, total);
  if (n) memcpy(offs_out, offs, 8 * n);
  free(offs);
  free(buf);
  return total;
}

}  // extern "C"

#ifdef BATCHCHECK_MAIN
// The packing cases of tests/test_batch_call_cpu.py, every source array allocated at exactly its
// size, and the plan's and the check's entry points once each.
static int g_bad = 0;
static void pack_case(const char* name, size_t data_bytes, std::vector<uint64_t> offsets,
                      std::vector<uint64_t> lengths) {
  const size_t n = offsets.size();
  uint8_t* data = data_bytes ? static_cast<uint8_t*>(malloc(data_bytes)) : nullptr;
  for (size_t i = 0; i < data_bytes; ++i) data[i] = (uint8_t)(7 + 31 * i);
  std::vector<uint8_t> want;
  std::vector<uint64_t> want_offs;
  for (size_t i = 0; i < n; ++i) {
    want_offs.push_back(want.size());
    for (uint64_t k = 0; k < lengths[i]; ++k) want.push_back(data[offsets[i] + k]);
  }
  std::vector<uint8_t> got(want.size());
  std::vector<uint64_t> got_offs(n);
  const uint64_t total = bc_pack(got.data(), got_offs.data(), data, n ? offsets.data() : nullptr,
                                 n ? lengths.data() : nullptr, n);
  if (total != want.size() || got != want || got_offs != want_offs) {
    fprintf(stderr, "pack case %s differs\n", name);
    ++g_bad;
  }
  free(data);
}

int main() {
  pack_case("empty set", 0, {}, {});
  pack_case("all empty, no data", 0, {0, 5, 9}, {0, 0, 0});
  pack_case("one run", 60, {0, 10, 30, 30}, {10, 20, 0, 30});
  pack_case("alternating gaps", 64, {0, 12, 20, 40, 63}, {8, 8, 10, 3, 1});
  pack_case("reversed", 40, {30, 20, 10, 0}, {10, 10, 10, 10});
  pack_case("overlapping", 32, {0, 4, 4, 0, 16}, {16, 16, 28, 32, 16});
  uint64_t o[16];
  bc_plan(3, 7, -1, 1, 1, 1000, 500, o);
  if (o[3] != 0 || o[4] != 256 || o[15] <= o[14]) ++g_bad;
  bc_plan(3, 7, 0, 0, 0, 1000, 0, o);
  if (o[0] != 0 || o[1] != 256 || o[13] + 256 != o[15]) ++g_bad;
  if (bc_check(0, 0, 0, 1.0, 0, 0, 0, 0, -1, 0, 0, 0, 1, 1, 1) != 0) ++g_bad;
  if (bc_check(0, 0, 0, 1.0, 0, 0, 1, 1, -1, 0, 0, 0, 1, 1, 1) == 0) ++g_bad;
  if (g_bad) return 1;
  printf("batchcheck ok\n");
  return 0;
}
#endif
