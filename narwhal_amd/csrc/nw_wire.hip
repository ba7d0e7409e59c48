// nw_wire.hip — wire ingest on the device: bincode PrimaryMessage frames, as one H2D copy put
// them into device memory, decoded into the structure-of-arrays the verification pipelines
// take (nw::rt::cert_pipeline / votes_pipeline). The per-frame decoder is nw_wiredec.hpp,
// shared with the CPU check (tools/wirecheck.hip).
//
//   k_wire_scan   one lane per frame: the walk that decides accept / reject is serial by
//                 nature (every field's position depends on the lengths before it), so a
//                 frame is one lane's work; the frame is read as aligned words plus a shift,
//                 one load per four bytes of key text. One wave per workgroup, so that a
//                 call of a few thousand frames still spreads over the CUs. Writes one
//                 32-byte record per frame (two 16-byte stores).
//   k_wire_emit   G lanes per frame (G = 16 or 64, the host picks by mean frame size): the
//                 frame's output is a list of 4-byte word tasks (header bytes, id, signature,
//                 then 24 words per vote: 8 decoded key words and 16 signature words), lane l
//                 takes tasks l, l + G, ...; contiguous lanes write contiguous words. Where
//                 each frame's rows go (its slot, header byte offset, first vote) comes from
//                 the host's prefix sums over the scan's records (nw_wireplace.hpp); the
//                 counts that drive the writes are the scan's own records in device memory,
//                 and every write is checked against the arrays' capacities.
//   k_wire_canon  (NW_WIRE_CANON_DEVICE) one workgroup per frame, between the scan and the
//                 read-back of its records: a Header / Certificate frame whose payload keys
//                 or parents are not strictly increasing gets the BTreeMap / BTreeSet sort
//                 and de-duplication as an order list (nw_wiredec.hpp, canon_*), its keys
//                 staged in LDS (36 bytes per entry with its kept flag, at most 36 KiB);
//                 every other frame's workgroup writes "not applicable" and exits. 64 or
//                 256 lanes per workgroup (the host picks by mean frame size: the walks
//                 are O(entries^2 / lanes)). k_wire_emit then reads such a frame through
//                 its order list (emit_lane<true>).
//
// These kernels move bytes: a few hundred to a few thousand per frame, no arithmetic beyond
// base64 (and, in k_wire_canon, key compares). The verification kernels that follow dominate
// the device time.
#include "nw_kernels.h"
#include "nw_wiredec.hpp"

namespace nw {

__global__ __launch_bounds__(64) void k_wire_scan(const uint32_t* __restrict__ frames,
                                                  const uint64_t* __restrict__ offsets,
                                                  uint64_t n, uint64_t total_bytes,
                                                  uint64_t max_frame,
                                                  wd::rec_t* __restrict__ recs) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t off = offsets[i], end = offsets[i + 1];
  wd::rec_t r{-1, 0, 0, 0, 0, 0, 0, 0};
  if (end >= off && end <= total_bytes) {   // (the host checked the offsets: belt and braces)
    const uint64_t len = end - off;
    if (len > max_frame) r.kind = wd::kOverCap;
    else r = wd::scan(frames, off, len);
  }
  uint4* o = reinterpret_cast<uint4*>(recs + i);
  o[0] = make_uint4((uint32_t)r.kind, r.canonical, r.np, r.nq);
  o[1] = make_uint4(r.nv, r.alen, r.vlen, 0u);
}

// kCanon: the instance that also serves canonicalised frames (a build of its own, so that the
// plain instance keeps its registers and occupancy).
template <uint32_t G, bool kCanon>
__global__ __launch_bounds__(256) void k_wire_emit(const uint32_t* __restrict__ frames,
                                                   const uint64_t* __restrict__ offsets,
                                                   uint64_t n, uint64_t total_bytes,
                                                   const wd::rec_t* __restrict__ recs,
                                                   const wd::dst_t* __restrict__ dsts,
                                                   const wd::canon_t* __restrict__ cans,
                                                   const uint32_t* __restrict__ order,
                                                   uint64_t order_cap, wd::out_t out) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t i = t / G;
  if (i >= n) return;
  const wd::dst_t d = dsts[i];
  if (d.slot == wd::kNoSlot) return;
  const uint64_t off = offsets[i], end = offsets[i + 1];
  if (end < off || end > total_bytes) return;
  const wd::rec_t r = recs[i];
  wd::emit_lane<kCanon>(frames, off, end - off, r, kCanon ? cans + i : nullptr, order,
                        order_cap, d, out, (uint32_t)(t % G), G);
}

// One workgroup of L lanes per frame. Every branch before a barrier depends on the frame
// alone, so the whole workgroup takes it together. LDS: 36 bytes per entry (8 key words and
// the kept flag) for lds_entries entries, which the host derives from the call's longest
// frame (an entry takes at least 32 frame bytes), so that calls of small frames are not held
// to the four workgroups per CU that the full 36 KiB allow.
template <uint32_t L>
__global__ __launch_bounds__(L) void k_wire_canon(const uint32_t* __restrict__ frames,
                                                    const uint64_t* __restrict__ offsets,
                                                    uint64_t n, uint64_t total_bytes,
                                                    const wd::rec_t* __restrict__ recs,
                                                    wd::canon_t* __restrict__ cans,
                                                    uint32_t* __restrict__ order,
                                                    uint64_t order_cap, uint32_t lds_entries) {
  extern __shared__ uint32_t lds[];
  uint32_t* keys = lds;
  uint32_t* kept = lds + 8 * (size_t)lds_entries;
  const uint64_t i = blockIdx.x;
  if (i >= n) return;
  const uint64_t off = offsets[i], end = offsets[i + 1];
  wd::canon_job_t jb;
  uint32_t state = wd::kCanonNone;
  if (end >= off && end <= total_bytes)
    state = wd::canon_begin(frames, off, end - off, recs[i], order_cap, &jb);
  if (state == wd::kCanonDone && jb.np + jb.nq > lds_entries)
    state = wd::kCanonNone;   // (not this call's bound: the host rejects the record)
  if (state != wd::kCanonDone) {
    if (threadIdx.x == 0)
      *reinterpret_cast<uint4*>(cans + i) = make_uint4(0u, 0u, state, 0u);
    return;
  }
  wd::canon_stage(threadIdx.x, L, jb, keys);
  __syncthreads();
  wd::canon_mark(threadIdx.x, L, jb, keys, kept);
  __syncthreads();
  wd::canon_rank(threadIdx.x, L, jb, keys, kept, order, cans + i);
}

hipError_t launch_wire_scan(const uint32_t* frames, const uint64_t* offsets, uint64_t n,
                            uint64_t total_bytes, uint64_t max_frame, wd::rec_t* recs,
                            hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const uint64_t blocks = (n + 63) / 64;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_wire_scan, dim3((unsigned)blocks), dim3(64), 0, stream, frames,
                     offsets, n, total_bytes, max_frame, recs);
  return hipGetLastError();
}

hipError_t launch_wire_emit(const uint32_t* frames, const uint64_t* offsets, uint64_t n,
                            uint64_t total_bytes, const wd::rec_t* recs, const wd::dst_t* dsts,
                            const wd::canon_t* cans, const uint32_t* order, uint64_t order_cap,
                            const wd::out_t& out, uint32_t group, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (group != 16 && group != 64) return hipErrorInvalidValue;
  const uint64_t blocks = (n * group + 255) / 256;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  auto k = group == 16 ? (cans ? k_wire_emit<16, true> : k_wire_emit<16, false>)
                       : (cans ? k_wire_emit<64, true> : k_wire_emit<64, false>);
  hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(256), 0, stream, frames, offsets, n,
                     total_bytes, recs, dsts, cans, order, order_cap, out);
  return hipGetLastError();
}

hipError_t launch_wire_canon(const uint32_t* frames, const uint64_t* offsets, uint64_t n,
                             uint64_t total_bytes, const wd::rec_t* recs, wd::canon_t* cans,
                             uint32_t* order, uint64_t order_cap, uint32_t lanes,
                             uint32_t lds_entries, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (lanes != 64 && lanes != 256) return hipErrorInvalidValue;
  if (lds_entries == 0 || lds_entries > wd::kCanonMax) return hipErrorInvalidValue;
  const size_t lds = 36 * (size_t)lds_entries;
  if (n > 0x7fffffffull) return hipErrorInvalidValue;
  if (lanes == 64)
    hipLaunchKernelGGL(k_wire_canon<64>, dim3((unsigned)n), dim3(64), lds, stream, frames,
                       offsets, n, total_bytes, recs, cans, order, order_cap, lds_entries);
  else
    hipLaunchKernelGGL(k_wire_canon<256>, dim3((unsigned)n), dim3(256), lds, stream, frames,
                       offsets, n, total_bytes, recs, cans, order, order_cap, lds_entries);
  return hipGetLastError();
}

}  // namespace nw
