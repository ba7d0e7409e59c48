// nw_batch_call.hpp — one verify_batch call as launch_verify_batch (nw_kernels.h) takes it, filled
// by field name, and the combinations of its options that are refused. Host only (plain C++,
// device memory behind opaque pointers): no kernel takes one.
#pragma once
#include <hip/hip_runtime_api.h>   // hipError_t
#include <stdint.h>

namespace nw {

struct z_key_t;
struct key_tables_t;
struct batch_votes_t;

// Input gate of a lone fused batch whose inputs the CPU is still writing into host-mapped
// device memory when the launch is queued (nw_jobs.cpp submit_batch): the head's vote waves
// wait until flags[vote / chunk] == seq (a system-scope load, then a system-scope acquire),
// so the kernels start while the bytes are in flight. digests and offsets must be written
// before the launch. chunk: a multiple of 64 votes.
struct input_gate_t {
  const uint32_t* flags;
  uint32_t seq;
  uint32_t chunk;
};

struct batch_call_t {
  // ---- inputs (device memory but host_offsets) ----
  // One 32-byte digest per batch; with `kplane`, the call's k plane: one row of 8 words per
  // vote, k_i = SHA-512(R_i || A_i || M_i) mod l (launch_strict_hram), memory the caller owns.
  const uint32_t* digests = nullptr;
  const uint64_t* offsets = nullptr;        // nbatches + 1 vote offsets
  const uint64_t* host_offsets = nullptr;   // the same values in host memory: plans the slices
  uint64_t nbatches = 0;
  const uint32_t* pks = nullptr;
  const uint32_t* sigs = nullptr;
  uint64_t nitems = 0;
  const uint32_t* z16 = nullptr;   // injected batch coefficients (optional)
  const z_key_t* zkey = nullptr;   // ChaCha20 key of the coefficients when z16 is null
  // ---- outputs ----
  int32_t* status = nullptr;
  uint64_t* fail_index = nullptr;
  void* workspace = nullptr;   // batch_workspace_bytes(nbatches, nitems)
  // ---- options ----
  // keys: pre-decompressed key tables with vote_key = per-item key index (certificate callers).
  const key_tables_t* keys = nullptr;
  // skip_group_ok (device): batch b is settled (status Ok) when
  // skip_group_ok[b / skip_per_group] != 0 (launch_cert_groups, launch_votes_keyed,
  // launch_batch_signers); active_frac: the caller's estimate of the fraction of votes not
  // skipped (chunk sizing).
  const uint32_t* skip_group_ok = nullptr;
  uint64_t skip_per_group = 0;
  double active_frac = 1.0;
  // skip_pip: with a skip list, batches of Pippenger size still take the Pippenger kernels, which
  // then honour the list (launch_batch_signers' callers); a lone large batch takes the separate
  // kernels, never the fused launches. Without it no batch of a call with a skip list takes the
  // Pippenger path (the certificate callers).
  bool skip_pip = false;
  // votes (with skip_pip, skip_per_group = 1, no key tables): the comb phase's verdict per vote
  // (launch_batch_signers, DESIGN.md 5 "Round 14"). A vote whose state is kVotePass adds nothing
  // to the sum of its batch for any coefficient set and cannot fail a check that comes before the
  // sum, so a batch that is sent on runs over its other votes only, each at its own position: the
  // items are built from the list, the Straus ladder runs over the chunks that hold a listed
  // vote, and in a Pippenger batch a passed vote is neutral and not decompressed.
  const batch_votes_t* votes = nullptr;
  // kplane: `digests` is the k plane, and the item and point kernels are the instances that read
  // k from it at the call-global vote index instead of hashing the batch digest.
  bool kplane = false;
  // ---- the fused lone batch's extras (verify_batch_outputs_direct) ----
  // fuse_ctr: a zeroed device array of verify_batch_fuse_ctr_bytes() (e.g. the job's own, left
  // zero by the tail), which saves the kernel that would zero the workspace's counters.
  uint32_t* fuse_ctr = nullptr;
  const input_gate_t* gate = nullptr;   // honoured by the fused head only (verify_batch_gate_ok)
  // done (host-mapped): the fused tail stores done_seq there (system scope) right after the
  // verdict, so a host may spin on it instead of waiting for the launch's completion signal.
  uint32_t* done = nullptr;
  uint32_t done_seq = 0;
};

// The combinations a plain (non-group) call is refused for (DESIGN.md 5 "Round 18" has the table;
// a batch larger than a workspace slice is refused in the slice loop). gate_ok / outputs_direct:
// verify_batch_gate_ok / verify_batch_outputs_direct of (nbatches, nitems).
inline hipError_t batch_call_check(const batch_call_t& c, bool gate_ok, bool outputs_direct) {
  const bool fused = c.fuse_ctr || c.gate || c.done;
  // over the k plane: never the fused launches, the plane must be there, plain batches only (no
  // key tables, no certificate skip list's compacted items)
  if (c.kplane && fused) return hipErrorInvalidValue;
  if (c.kplane && c.nbatches && c.nitems && !c.digests) return hipErrorInvalidValue;
  if (c.kplane && (c.keys || fused || c.active_frac < 1.0 || (c.skip_group_ok && !c.skip_pip)))
    return hipErrorInvalidValue;
  // Pippenger batches under a skip list take the separate kernels only: the fused launches order
  // themselves by tickets and counters, and a block that left early would leave another waiting
  if (c.skip_pip && (!c.skip_group_ok || fused)) return hipErrorInvalidValue;
  // the comb phase's vote list: its callers' plain batches only (a vote's state says nothing
  // about a keyed item, and the list's indices are 32 bits)
  if (c.votes && (!c.skip_pip || c.skip_per_group != 1 || c.keys || c.active_frac < 1.0 ||
                  c.nitems > 0xffffffffull))
    return hipErrorInvalidValue;
  // a gate is honoured by the fused head only: refuse it anywhere else (its waves would read
  // bytes the CPU has not written yet)
  if (c.gate && !gate_ok) return hipErrorInvalidValue;
  if (c.gate && (c.gate->chunk == 0 || c.gate->chunk % 64 != 0)) return hipErrorInvalidValue;
  if (c.done && !outputs_direct) return hipErrorInvalidValue;
  // the Pippenger launches over the plane take neither gate nor done word
  if (c.kplane && (c.gate || c.done)) return hipErrorInvalidValue;
  return hipSuccess;
}

}  // namespace nw
