// nw_strict_keymajor.hpp — key-major order of a strict launch's slice (DESIGN.md 5 "Round 16"):
// the third device region of an unkeyed two-pass launch, beside the two of nw_strict_layout.hpp,
// and the pure functions that map an item's key index to its bin. The launcher, the counters'
// reader and the host-only tools share this description. Plain C++ (and device code).
//
// The comb kernels gather 32 of an item's 43 table entries from its key's 528 KB of 8-bit
// tables. In item order a wave's 64 lanes name 64 keys, so with a few thousand hot keys every
// one of those reads is a random 128-byte gather over gigabytes. A counting sort of the slice's
// items by key index (k_km_hist / k_km_scan / k_km_scatter, after the certificate votes'
// k_vk_*) puts lane p on item perm[p], so that the lanes resident at one time span a few dozen
// keys whose tables stay in the last-level caches. Bins are GROUPS of 2^shift consecutive key
// indices: what the caches see is set by how many keys the resident lanes span, not by whether a
// wave holds one key or eight, and at most kKmBins bins fit the 4 KB LDS histogram and keep the
// global atomics (one per block and bin used) a few hundred thousand per pass.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define NW_KM_HD __host__ __device__ inline
#else
#define NW_KM_HD inline
#endif

namespace nw {

constexpr uint32_t kKmBins = 1024;     // key groups, then the one last bin of items without a key
constexpr uint32_t kKmChunk = 16384;   // consecutive items a block of the sort takes
constexpr uint64_t kKmBlockBytes = 256;

// The key indices of a slice are 0 .. space - 1 (the registry's rows first, then the call-local
// tables: k_strict_comb_select). The smallest shift at which they fall into at most
// kKmBins - 1 groups.
NW_KM_HD uint32_t km_shift(uint32_t space) {
  uint32_t s = 0;
  while (space != 0 && ((space - 1) >> s) >= kKmBins - 1) ++s;
  return s;
}
// The bin of an item whose key index is kk (kNoKey, or any index >= space: no live key, the
// last bin, whose lanes do no comb work).
NW_KM_HD uint32_t km_bin(uint32_t kk, uint32_t space, uint32_t shift) {
  return kk < space ? kk >> shift : kKmBins - 1;
}
// The region's block: the slice's words (written by k_km_scan when the slice is sorted, read by
// nobody otherwise), then the launch's counters (diagnostics, kept over its slices). The whole
// block and both histograms are cleared once per launch; k_km_scan leaves the histogram zero.
struct km_block_t {
  uint32_t npos;     // positions that hold an item with a live key
  uint32_t pad0_;
  unsigned long long placed;   // items with a live key that the sort placed
  unsigned long long bins;     // key bins that held an item
  unsigned long long slices;   // slices sorted
  unsigned char pad1_[kKmBlockBytes - 32];
};
static_assert(offsetof(km_block_t, npos) == 0 && offsetof(km_block_t, placed) == 8 &&
                  offsetof(km_block_t, bins) == 16 && offsetof(km_block_t, slices) == 24 &&
                  sizeof(km_block_t) == kKmBlockBytes,
              "the kernels and the counters' reader share these offsets");

// The block, the histogram and the cursors (kKmBins words each), then per position of the slice
// the item there (perm) and that item's slot in the slice's key set (pslot, so that a comb lane
// reads its slot at its own position).
struct km_region_t {
  uint64_t hist, cursor, perm, pslot, bytes;
};
inline km_region_t km_region_plan(uint64_t slice) {
  km_region_t r;
  r.hist = kKmBlockBytes;
  r.cursor = r.hist + 4 * (uint64_t)kKmBins;
  r.perm = r.cursor + 4 * (uint64_t)kKmBins;
  r.pslot = r.perm + 4 * slice;
  r.bytes = r.pslot + 4 * slice;
  return r;
}
constexpr uint64_t kKmClearBytes = kKmBlockBytes + 2 * 4 * (uint64_t)kKmBins;   // block, hist, cursor
// Empty (every member null) for a launch in item order.
struct km_region_view {
  km_block_t* block = nullptr;
  uint32_t *hist = nullptr, *cursor = nullptr, *perm = nullptr, *pslot = nullptr;
  km_region_view() = default;
  km_region_view(void* b, const km_region_t& r)
      : block(reinterpret_cast<km_block_t*>(b)),
        hist(reinterpret_cast<uint32_t*>(static_cast<char*>(b) + r.hist)),
        cursor(reinterpret_cast<uint32_t*>(static_cast<char*>(b) + r.cursor)),
        perm(reinterpret_cast<uint32_t*>(static_cast<char*>(b) + r.perm)),
        pslot(reinterpret_cast<uint32_t*>(static_cast<char*>(b) + r.pslot)) {}
};

}  // namespace nw
