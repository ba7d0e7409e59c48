// nw_strict_layout.hpp — the two device regions of an unkeyed two-pass strict launch
// (launch_verify_strict) and the blocks of words and counters at fixed places in them: the one
// description that the launcher, the counters' reader and the host-only tools share. Plain C++.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace nw {

struct ge_cached_pk;   // nw_strict.hpp
struct ge_niels_pad;   // nw_point.hpp

// ---- the triage region: the slice's planes, list and key set ----
constexpr uint64_t kTriagePlaneCount = 42, kKeyTabBytes = 1024, kTriageBlockBytes = 2048;
constexpr uint32_t kKeyStatLanes = 128;
// The region's block: the slice's words, cleared before every slice, then the launch's counters
// (diagnostics, kept over its slices), cleared once per launch that has a key set.
struct triage_block_t {
  uint32_t count;   // the slice's list entries (k_strict_triage)
  uint32_t nkeys;   // the slice's distinct keys with a slot (k_strict_keys_probe)
  unsigned long long keys_tabulated;   // k_strict_keys_build
  unsigned char pad_[1024 - 16];
  // items with a slot, spread so that the blocks of k_strict_keys_probe do not queue on one address
  unsigned long long with_slot[kKeyStatLanes];
};
constexpr size_t kTriageSliceWordsBytes = offsetof(triage_block_t, keys_tabulated);
static_assert(offsetof(triage_block_t, count) == 0 && offsetof(triage_block_t, nkeys) == 4 &&
                  offsetof(triage_block_t, keys_tabulated) == 8 &&
                  offsetof(triage_block_t, with_slot) == 1024 &&
                  sizeof(triage_block_t) == kTriageBlockBytes,
              "the kernels and the counters' reader share these offsets");

// Byte offsets of the region's parts for a slice (a multiple of 64 items) and key_slots slots
// (0: no key set): kTriagePlaneCount planes, the list and the key-slot plane (a word per item
// each), the block, then the key set: slots and flags (a word per slot each), 256 bytes of
// padding, and the tables (kKeyTabBytes per slot; 256-byte aligned, since every term before them
// is a multiple of 256).
struct strict_region_t {
  uint64_t list, keyslot, block, slots, kflags, ktabs, bytes;
};
inline strict_region_t strict_region_plan(uint64_t slice, uint64_t key_slots) {
  strict_region_t r;
  r.list = 4 * kTriagePlaneCount * slice;
  r.keyslot = r.list + 4 * slice;
  r.block = r.keyslot + 4 * slice;
  r.slots = r.block + kTriageBlockBytes;
  r.kflags = r.slots + 4 * key_slots;
  r.ktabs = r.kflags + 4 * key_slots + 256;
  r.bytes = r.ktabs + kKeyTabBytes * key_slots;
  return r;
}
template <class T>
inline T* region_part(void* base, uint64_t offset) {
  return reinterpret_cast<T*>(static_cast<char*>(base) + offset);
}
struct strict_region_view {
  uint32_t *planes, *list, *keyslot;   // keyslot: null without a key set, the kernels' test for it
  triage_block_t* block;
  uint32_t *slots, *kflags;
  ge_cached_pk* ktabs;
  strict_region_view(void* b, const strict_region_t& r, bool key_set)
      : planes(region_part<uint32_t>(b, 0)), list(region_part<uint32_t>(b, r.list)),
        keyslot(key_set ? region_part<uint32_t>(b, r.keyslot) : nullptr),
        block(region_part<triage_block_t>(b, r.block)), slots(region_part<uint32_t>(b, r.slots)),
        kflags(region_part<uint32_t>(b, r.kflags)), ktabs(region_part<ge_cached_pk>(b, r.ktabs)) {}
};

// ---- the comb path's region: the hot keys' tables, per-slot words, the to-do list ----
constexpr uint64_t kCombBlockBytes = 2048;
constexpr uint32_t kCombStatLanes = 32;
// Its block: the slice's words, cleared before every slice, then the launch's counters
// (diagnostics), cleared once per launch; the lane_ arrays take one atomic per block or wave,
// spread over kCombStatLanes addresses, and are summed by the reader.
struct comb_block_t {
  uint32_t nhot;         // hot keys of the slice; may end above hot_cap, its readers clamp it
  uint32_t todo_count;   // entries of the to-do list
  uint32_t nlive;        // hot keys + registered keys in the slice
  uint32_t pad0_;
  unsigned long long hot_keys;    // k_strict_comb_select
  unsigned long long checked;     // k_strict_keyed<true> (no registry)
  unsigned long long listed;      // items that came to the triage
  unsigned long long matched;     // registered keys that occurred (k_strict_signers_match)
  unsigned long long laddered;    // items handed to k_verify_strict_pre
  unsigned char pad1_[1024 - 56];
  unsigned long long lane_checked[kCombStatLanes];      // k_strict_signers_count: items checked,
  unsigned long long lane_reg_items[kCombStatLanes];    // of them under a registered key,
  unsigned long long lane_reg_passed[kCombStatLanes];   // of those passed
  unsigned long long lane_settled[kCombStatLanes];      // the triage's equation failures
};
constexpr size_t kCombSliceWordsBytes = offsetof(comb_block_t, hot_keys);
static_assert(offsetof(comb_block_t, nhot) == 0 && offsetof(comb_block_t, todo_count) == 4 &&
                  offsetof(comb_block_t, nlive) == 8 && offsetof(comb_block_t, hot_keys) == 16 &&
                  offsetof(comb_block_t, checked) == 24 && offsetof(comb_block_t, listed) == 32 &&
                  offsetof(comb_block_t, matched) == 40 && offsetof(comb_block_t, laddered) == 48 &&
                  offsetof(comb_block_t, lane_checked) == 1024 &&
                  offsetof(comb_block_t, lane_reg_items) == 1280 &&
                  offsetof(comb_block_t, lane_reg_passed) == 1536 &&
                  offsetof(comb_block_t, lane_settled) == 1792 &&
                  sizeof(comb_block_t) == kCombBlockBytes,
              "the kernels and the counters' reader share these offsets");

// The block, the to-do list (a word per item of the slice), per slot of the key set its uses,
// its hot index and its registry row, per hot key its owner's row and its flags, then the
// tables: tabs_bytes = key_tables_bytes(hot_cap, keyspec_for(8)).
struct comb_region_t {
  uint64_t todo, uses, hotidx, match, hotrow, hok, tabs, bytes;
};
inline comb_region_t comb_region_plan(uint64_t slice, uint64_t key_slots, uint64_t hot_cap,
                                      uint64_t tabs_bytes) {
  comb_region_t r;
  r.todo = kCombBlockBytes;
  r.uses = r.todo + 4 * slice;
  r.hotidx = r.uses + 4 * key_slots;
  r.match = r.hotidx + 4 * key_slots;
  r.hotrow = r.match + 4 * key_slots;
  r.hok = r.hotrow + 4 * hot_cap;
  r.tabs = (r.hok + 4 * hot_cap + 255) & ~255ull;
  r.bytes = r.tabs + tabs_bytes;
  return r;
}
// Empty (every member null) for a launch without the path.
struct comb_region_view {
  comb_block_t* block = nullptr;
  uint32_t *todo = nullptr, *uses = nullptr, *hotidx = nullptr, *match = nullptr;
  uint32_t *hotrow = nullptr, *hok = nullptr;
  ge_niels_pad* tabs = nullptr;
  comb_region_view() = default;
  comb_region_view(void* b, const comb_region_t& r)
      : block(region_part<comb_block_t>(b, 0)), todo(region_part<uint32_t>(b, r.todo)),
        uses(region_part<uint32_t>(b, r.uses)), hotidx(region_part<uint32_t>(b, r.hotidx)),
        match(region_part<uint32_t>(b, r.match)), hotrow(region_part<uint32_t>(b, r.hotrow)),
        hok(region_part<uint32_t>(b, r.hok)), tabs(region_part<ge_niels_pad>(b, r.tabs)) {}
};

}  // namespace nw
