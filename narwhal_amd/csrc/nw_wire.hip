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
//                 the host's prefix sums over the scan's records; the counts that drive the
//                 writes are the scan's own records in device memory, and every write is
//                 checked against the arrays' capacities.
//
// These kernels move bytes: a few hundred to a few thousand per frame, no arithmetic beyond
// base64. The verification kernels that follow dominate the device time.
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

template <uint32_t G>
__global__ __launch_bounds__(256) void k_wire_emit(const uint32_t* __restrict__ frames,
                                                   const uint64_t* __restrict__ offsets,
                                                   uint64_t n, uint64_t total_bytes,
                                                   const wd::rec_t* __restrict__ recs,
                                                   const wd::dst_t* __restrict__ dsts,
                                                   wd::out_t out) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t i = t / G;
  if (i >= n) return;
  const wd::dst_t d = dsts[i];
  if (d.slot == wd::kNoSlot) return;
  const uint64_t off = offsets[i], end = offsets[i + 1];
  if (end < off || end > total_bytes) return;
  const wd::rec_t r = recs[i];
  wd::emit_lane(frames, off, end - off, r, d, out, (uint32_t)(t % G), G);
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
                            const wd::out_t& out, uint32_t group, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (group != 16 && group != 64) return hipErrorInvalidValue;
  const uint64_t blocks = (n * group + 255) / 256;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  if (group == 16)
    hipLaunchKernelGGL(k_wire_emit<16>, dim3((unsigned)blocks), dim3(256), 0, stream, frames,
                       offsets, n, total_bytes, recs, dsts, out);
  else
    hipLaunchKernelGGL(k_wire_emit<64>, dim3((unsigned)blocks), dim3(256), 0, stream, frames,
                       offsets, n, total_bytes, recs, dsts, out);
  return hipGetLastError();
}

}  // namespace nw
