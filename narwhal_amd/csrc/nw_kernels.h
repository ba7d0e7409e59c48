// nw_kernels.h — launchers for the gfx950 kernels (host side of nw_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "narwhal_amd.h"
#include "nw_batch_call.hpp"
#include "nw_strict_layout.hpp"
#include "nw_strict_keymajor.hpp"

namespace nw {

struct z_key_t {
  uint32_t key[8];
  uint64_t nonce;
};

// Computes the curve constants and the B table on the host (from their definitions) and
// copies them to the current device's constant memory.
hipError_t upload_consts();

// hipMalloc for the large per-device tables (strict B tables, keyed B comb, committee key
// tables, strict workspace). Test hook: NW_DEVICE_MEM_LIMIT=bytes makes any such allocation
// above that size fail with hipErrorOutOfMemory, as on a device without the memory.
hipError_t table_malloc(void** p, size_t bytes);

// lengths == nullptr: offsets has n + 1 entries and message i = [offsets[i], offsets[i+1]).
hipError_t launch_sha512_digest32(const uint8_t* data, const uint64_t* offsets,
                                  const uint64_t* lengths, uint64_t n, uint32_t* out,
                                  hipStream_t stream);

// Strict verification; workspace = strict_workspace_bytes() of device memory (per-lane
// tables; reusable across launches on one stream).
size_t strict_workspace_bytes();
// The two-pass path (unkeyed launches, NW_STRICT_TRIAGE) also needs a region of
// strict_triage_bytes(slice, key_slots) for a slice of strict_triage_slice(n) items: per item
// the x of A and R (20 words), the ladder's digit words, vneg and window count (22), a list
// entry and a key slot, then the slice's key set (strict_keys_slots).
// strict_triage_slice(n) = min(slice limit, n rounded up to 64); the limit is 2^24 items
// (NW_TRIAGE_SLICE = items lowers it, e.g. to run a small input through several slices);
// 0 when the two-pass path is off.
uint64_t strict_triage_slice(uint64_t n, bool always = false);
// The slice's key set: the items of a slice share public keys, so each distinct key is
// decompressed and tabulated once per slice into a table that lives for the call only.
// strict_keys_slots(slice) = slots of its hash table for a slice of that many items, from
// NW_STRICT_KEYS (read per launch; 0 = off); strict_keys_plan is the pure sizing rule.
// Slots are clamped to [64, 2^20], rounded up to a power of two (default 2^16: 64 MB of
// tables) and to no more than 4 x the slice's items (every key of the slice then fills at most
// a quarter of them: short probe chains); at most half of them are filled.
constexpr uint64_t kKeySlotsDefault = 1ull << 16, kKeySlotsMin = 64, kKeySlotsMax = 1ull << 20;
inline uint64_t strict_keys_plan(uint64_t requested, uint64_t slice) {
  if (requested == 0 || slice == 0) return 0;
  uint64_t want = requested < kKeySlotsMin ? kKeySlotsMin
                : requested > kKeySlotsMax ? kKeySlotsMax : requested;
  const uint64_t fill = 4 * slice < kKeySlotsMin ? kKeySlotsMin : 4 * slice;
  if (want > fill) want = fill;
  uint64_t cap = kKeySlotsMin;
  while (cap < want) cap <<= 1;
  return cap;
}
uint64_t strict_keys_slots(uint64_t slice);
// The region for a slice of that many items and key_slots slots (nw_strict_layout.hpp
// strict_region_plan).
size_t strict_triage_bytes(uint64_t slice, uint64_t key_slots);
// The device's registered signers (DESIGN.md 5 "Round 10", nw_strict.hpp signers_lookup): n
// distinct keys whose 8-bit comb tables (keyspec_for(8), identity rows, no lambda: the layout
// and flags of a launch's call-local tables) are kept until the set is replaced, in one
// allocation of their own (base). Their items take the comb check whatever the launch's size;
// a registered key that does not decode or has small order is never matched. The same tables
// serve the plain batches (launch_batch_signers), which also need each key's lambda.
struct strict_signers_t {
  void* base = nullptr;
  const uint32_t* keys = nullptr;    // n x 8 words
  const uint32_t* slots = nullptr;   // cap words: row + 1 or 0
  const uint32_t* ok = nullptr;      // n flag words (kKeyDecoded, kKeySmall)
  const uint32_t* lam = nullptr;     // n words: lambda with [l]A == [lambda]T8 (0: no torsion
                                     // component, or the key does not decode); kept out of `ok`,
                                     // whose words the strict launches read as they are
  const struct ge_niels_pad* tabs = nullptr;
  uint32_t n = 0, cap = 0;
};
// Builds the registry of the n distinct keys at keys32 (host memory, 32 bytes each) on the
// current device: allocates (table_malloc), uploads the keys and the host-built hash table and
// queues the table build on `stream`; the host buffers are free once it returns. n = 0 gives the
// empty registry. hipErrorInvalidValue when no hash table holds the keys (more than kKeyProbes
// keys of one hash); on any error *out is empty and nothing is left allocated.
hipError_t strict_signers_build(const uint8_t* keys32, uint32_t n, strict_signers_t* out,
                                hipStream_t stream);
void strict_signers_free(strict_signers_t* sg);
// Registered keys a device takes (NW_STRICT_SIGNERS_MAX, default 8192: 4.3 GB of tables) and the
// items from which a launch uses them (NW_STRICT_SIGNERS_MIN_ITEMS); both read at the call.
uint64_t strict_signers_max();
uint64_t strict_signers_min_items();
// For the last unkeyed two-pass launch queued on the current device: registered keys that
// occurred in it (summed over its slices), items checked under them, items the comb passed under
// them. Synchronises `stream`.
hipError_t strict_signers_stats(uint64_t out[3], hipStream_t stream);
// One launch's plan (the knobs, read once per launch: NW_TRIAGE_SLICE, NW_STRICT_KEYS,
// NW_STRICT_COMB / _MIN / _KEYS, NW_STRICT_SIGNERS_MIN_ITEMS, NW_STRICT_COMB_DECIDE,
// NW_STRICT_KEY_MAJOR) for n items
// on a device with `registered` registered signers. n = 0 (a keyed launch), or the two-pass
// path off: the empty plan.
struct strict_launch_plan_t {
  uint64_t slice = 0;        // items per slice (strict_triage_slice(n))
  uint64_t key_slots = 0;    // strict_keys_slots(slice); 0: no key set
  uint64_t hot_cap = 0;      // hot keys per slice; 0: no call-local tables
  uint32_t comb_min = 0;     // uses from which a key is hot
  bool signers = false;      // the registered signers are used
  bool comb_decide = true;   // the to-do entries carry the comb's verdict
  // the comb path runs: with registered signers even without room for a call-local table
  bool comb() const { return hot_cap != 0 || signers; }
  // Key-major order of the comb path's lanes (nw_strict_keymajor.hpp; NW_STRICT_KEY_MAJOR, read
  // per launch: 0 = item order, the kernel sequence without the sort; 1 = every slice is sorted;
  // unset = the host's part of the decision here, slice >= kKmAutoSlice, and the device's in
  // the kernels, live keys of the slice >= km_min_live).
  bool key_major = false;
  uint32_t km_min_live = 0;
};
// The automatic decision's thresholds (DESIGN.md 5 "Round 16" has the rows behind them): the
// smallest slice and the fewest live keys at which the sorted launch measured faster (2^20
// items under 4,096 keys: 8.52 -> 7.75 ms; 12.5M under 64: 25.4 -> 23.6 ms); 65,536 items
// measured no gain under 4,096 keys and 2 % slower under 64, fewer than 64 keys were not measured.
constexpr uint64_t kKmAutoSlice = 1ull << 20;
constexpr uint32_t kKmAutoLive = 64;
size_t strict_keymajor_bytes(uint64_t slice);
// For the last unkeyed two-pass launch queued on the current device: items with a live key that
// the sort placed, key bins that held an item, slices sorted (each summed over the slices); all 0
// for a launch in item order. Synchronises `stream`.
hipError_t strict_keymajor_stats(uint64_t out[3], hipStream_t stream);
// always: plan the two-pass launch whatever NW_STRICT_TRIAGE says (launch_verify_strict_msgs).
strict_launch_plan_t strict_launch_plan(uint64_t n, uint32_t registered, bool always = false);
// What Lease::strict_ws hands a launch: the allocations, what they hold and the launch's plan.
struct strict_caps_t {
  uint64_t slice = 0, key_slots = 0;   // triage: strict_triage_bytes(slice, key_slots)
  uint64_t hot_keys = 0;               // comb: strict_comb_bytes(slice, key_slots, hot_keys)
  uint64_t km_slice = 0;               // key-major order: strict_keymajor_bytes(km_slice)
};
struct strict_ws_t {
  void* base = nullptr;       // strict_workspace_bytes()
  void* triage = nullptr;     // null for a keyed launch
  void* comb = nullptr;       // null: the launch runs without the comb path
  void* keymajor = nullptr;   // null: the launch runs in item order
  strict_caps_t caps;
  strict_launch_plan_t plan;  // without comb: hot_cap = 0 and signers = false
  strict_signers_t signers;   // the device's registered signers when plan.signers (else n == 0)
  uint32_t* kplane = nullptr; // launch_verify_strict_msgs only: 8 words per item of the call
};
// The comb check for a call's hot keys (DESIGN.md 5 "Round 9"): a key of the slice's set used
// by at least NW_STRICT_COMB_MIN items (default 256) that decodes and is not small gets 8-bit
// comb tables j * 2^(8 t) A (keyspec_for(8): 32 tables of 129 entries, 528 KB) for the call,
// and its items run keyed_vote_check_ex (additions only, R never decompressed); everything the
// check does not pass goes through the triage from a compacted list. An item that left the
// check before its comb sum then takes the ladder as before; one whose sum ran and gave
// R' != decode(R) carries that verdict in its list entry, and the triage settles it (R does not
// decode, or NW_ERR_EQUATION) without the ladder (NW_STRICT_COMB_DECIDE=0, read per launch:
// every listed item takes the ladder again). NW_STRICT_COMB=0 turns the path off; hot keys per slice are limited to
// hot_cap = min(NW_STRICT_COMB_KEYS (default 8192), slice / min). All three are read per
// launch. The path's allocation (tables, per-slot counts and indices, the to-do list) is
// apart from the triage region's.
size_t strict_comb_bytes(uint64_t slice, uint64_t key_slots, uint64_t hot_cap);
// For the last unkeyed two-pass launch queued on the current device: hot keys tabulated, items
// checked by the comb, items it passed, items sent on to the triage. Synchronises `stream`.
hipError_t strict_comb_stats(uint64_t out[4], hipStream_t stream);
// Of the items sent on, for the same launch (DESIGN.md 5 "Round 11"): items the triage settled as
// NW_ERR_EQUATION from the comb's verdict, items handed to the ladder (k_verify_strict_pre). Both
// 0 when the comb path was off. Synchronises `stream`.
hipError_t strict_decided_stats(uint64_t out[2], hipStream_t stream);
// For the last unkeyed two-pass launch queued on the current device: distinct keys tabulated,
// items that read a shared table, items on their own path. Synchronises `stream`.
hipError_t strict_keyset_stats(uint64_t out[3], hipStream_t stream);
// keys (optional): pre-decompressed key tables with vote_key = per-item key index.
// Builds the current device's lazily built strict tables (nw_prepare).
hipError_t prepare_strict_tables();
hipError_t launch_verify_strict(const uint32_t* msgs, uint32_t msg_stride_words,
                                const uint32_t* pks, const uint32_t* sigs, uint64_t n,
                                int32_t* status, uint64_t* bitmap, const strict_ws_t& workspace,
                                hipStream_t stream, const struct key_tables_t* keys = nullptr);

// The same over messages of any length (Ed25519 verify_strict over &[u8]): message i is lengths[i]
// bytes at data + offsets[i] (device arrays; any alignment). k_strict_hram writes k = SHA-512(R ||
// A || M) mod l of every item into workspace.kplane (the library's: 32 bytes per item, stride 8
// words, the shape of a digests array), then the unkeyed two-pass launch runs over the plane with
// the instances of its kernels that read k instead of hashing 32 bytes: key set, call-local
// comb, registered signers, to-do list, triage with decided items, ladder, bitmap and slices,
// under the same knobs and counted by the same statistics. Always two passes: NW_STRICT_TRIAGE=0
// is not honoured (workspace.plan comes from strict_launch_plan(n, registered, true)).
hipError_t launch_verify_strict_msgs(const uint8_t* data, const uint64_t* offsets,
                                     const uint64_t* lengths, const uint32_t* pks,
                                     const uint32_t* sigs, uint64_t n, int32_t* status,
                                     uint64_t* bitmap, const strict_ws_t& workspace,
                                     hipStream_t stream);

// k_strict_hram alone, for the launchers of other translation units (launch_verify_batch_msgs,
// launch_batch_signers' callers): k = SHA-512(R || A || M) mod l of items 0..n-1 into kplane + 8 i.
// One lane per item; a wave runs as long as its longest message.
hipError_t launch_strict_hram(const uint8_t* data, const uint64_t* offsets,
                              const uint64_t* lengths, const uint32_t* pks, const uint32_t* sigs,
                              uint64_t n, uint32_t* kplane, hipStream_t stream);

hipError_t launch_keypair(const uint32_t* seeds, uint64_t n, uint32_t* pks, hipStream_t stream);

hipError_t launch_sign(const uint32_t* sks, uint32_t sk_stride_words, const uint32_t* msgs,
                       uint32_t msg_stride_words, uint64_t n, uint32_t* sigs,
                       hipStream_t stream);

// k_sign_msgs: RFC 8032 signatures over messages of any length. Message i is lengths[i] bytes at
// data + offsets[i] (device arrays; any alignment; data may be null when every message is empty);
// sks as launch_sign takes them (seed || public key, stride 16 words, or 0 = one key for every
// message). Both hashes run on the item's lane over the message itself, which is read twice. One
// lane per item, and a wave runs as long as its longest message: meant for messages of up to a
// few KB, like launch_strict_hram.
hipError_t launch_sign_msgs(const uint32_t* sks, uint32_t sk_stride_words, const uint8_t* data,
                            const uint64_t* offsets, const uint64_t* lengths, uint64_t n,
                            uint32_t* sigs, hipStream_t stream);

// crypto::Signature::verify_batch over many batches (nw_batch.hip). offsets: device copy,
// host_offsets: the same nbatches + 1 values in host memory (used to plan the chunks and
// the workspace slices).
hipError_t upload_batch_consts();

// Layout of a committee's key comb tables at digit width W (chosen per committee when its
// tables are built: nw_api.cpp key_width): ntab = ceil(253 / W) comb tables j * 2^(W t) A,
// j = 0..2^(W-1) (affine niels), k's digits signed except the top one when ntab W > 256;
// the keyed vote chunks' second 8-bit table j * 2^128 A is comb table 128 / W when W divides
// 128, else one more table built from 2^128 A. W = 16: 16 tables, 67 MB per key; W = 20:
// 13 + 1 tables, 940 MB per key; W = 24 (NW_KEY_WIDTH=24 only): 11 tables.
// Only these three widths are built for a committee (nw_api.cpp key_width /
// alloc_key_tables); W = 8 (32 tables of 129 entries, every digit signed, 528 KB per key) is
// the width of the call-local tables of a strict launch's hot keys (strict_launch_plan) and of
// nothing else. Any other W (e.g. the 0 of a device without tables) is mapped to 16, so that
// no caller can divide by zero or shift by W - 1 < 0 here, on the host or the device.
#define NW_KS __host__ __device__ __forceinline__
struct keyspec {
  uint32_t W, ntab, nsigned, nent, tab, half;
  uint32_t bias[8];   // k + bias: the recoded digit words (2^(W-1) per signed digit)
};
NW_KS constexpr keyspec keyspec_for(uint32_t W) {
  keyspec ks{};
  if (W != 8 && W != 16 && W != 20 && W != 24) W = 16;
  ks.W = W;
  ks.ntab = (253 + W - 1) / W;
  ks.nsigned = ks.ntab * W > 256 ? ks.ntab - 1 : ks.ntab;
  ks.nent = (1u << (W - 1)) + 1;
  const uint32_t extra = 128 % W ? 1u : 0u;
  ks.tab = (ks.ntab + extra) * ks.nent;
  ks.half = (extra ? ks.ntab : 128 / W) * ks.nent;
  for (uint32_t m = 0; m < ks.nsigned; ++m) {
    const uint32_t b = W * m + W - 1;
    ks.bias[b >> 5] |= 1u << (b & 31);
  }
  return ks;
}
NW_KS constexpr uint32_t keyspec_tables(const keyspec& ks) { return ks.tab / ks.nent; }

// Pre-decompressed public keys (a committee): per key its comb tables (layout ks) and
// whether it decompressed. vote_key[i] = key index of vote i, or kNoKey to decompress that
// vote's key in the kernel (the verdict semantics are unchanged: a key's decompression is
// deterministic). Keyed strict verifications take [k]A from the ntab tables with no
// doublings; chunks whose votes are all keyed run 8-bit A windows over the tables of j * A
// and j * 2^128 A (entries 0..128) and a 128-doubling ladder.
struct key_tables_t {
  const struct ge_niels_pad* tabs;   // nkeys x ks.tab, affine niels (mixed additions)
  const uint32_t* ok;             // nkeys
  const uint32_t* vote_key;       // nitems (global item index)
  keyspec ks;
};
constexpr uint32_t kNoKey = 0xffffffffu;
constexpr uint32_t kKeyWMax = 24;   // widths 16 / 20 / 24 (at most 16 comb digits), and 8 (32)
constexpr uint32_t kKeyRun = 64, kKeyRun8 = 43;   // entries per lane of k_key_tabs (129 = 3 x 43)
// ok[key]: bit 0 = decompressed, bit 1 = small order (8A == identity), bits 2..4 = lambda
// with [l]A == [lambda]T8 (nw_strict.hpp kKeyLambdaShift: the key's torsion image)
size_t key_tables_bytes(uint64_t nkeys, const keyspec& ks);
// tabs: key_tables_bytes(nkeys) of device memory; ok: nkeys words. saved (nkeys x 8 words)
// and flag (1 word), optional: the keys the tables were last built from; the tables are
// rebuilt only when force or the keys differ (a device-side compare, so the call stays
// asynchronous), and saved is updated — the committee of an epoch is tabulated once.
hipError_t launch_key_tables(const uint32_t* pks, uint64_t nkeys, const keyspec& ks,
                             struct ge_niels_pad* tabs, uint32_t* ok, hipStream_t stream,
                             uint32_t* saved = nullptr, uint32_t* flag = nullptr,
                             bool force = true);
// The same for keys named by row: key i is pks[8 rows[i]..], i < min(*nlive, ncap) (both read
// on the device; the grids are sized for ncap). No lambda is computed (ok = decoded / small
// order only): for the strict check of a call's hot keys, any width keyspec_for builds.
hipError_t launch_key_tables_rows(const uint32_t* pks, const uint32_t* rows,
                                  const uint32_t* nlive, uint64_t ncap, const keyspec& ks,
                                  struct ge_niels_pad* tabs, uint32_t* ok, hipStream_t stream);
// lam[i] = lambda of key i (nw_strict.hpp key_lambda; 0 when it does not decode), one lane per key.
hipError_t launch_key_lambda(const uint32_t* pks, uint64_t nkeys, uint32_t* lam,
                             hipStream_t stream);
size_t batch_workspace_bytes(uint64_t nbatches, uint64_t nitems);
// True when launch_verify_batch over these batches (no skip list, no fork) writes its outputs
// from ONE kernel, the fused tail of a lone large batch: status / fail_index may then be
// host-mapped (fine-grained) memory, written in place, with no copy back.
bool verify_batch_outputs_direct(uint64_t nbatches, uint64_t nitems);
// Bytes of the fused launches' counters; a caller on that path may pass launch_verify_batch
// a zeroed device array of this size (fuse_ctr, e.g. shipped with its inputs' H2D copy),
// which saves the kernel that would zero them.
size_t verify_batch_fuse_ctr_bytes();
// verify_batch_gate_ok: the batch takes the fused head, the only launch that honours an input
// gate (nw_batch_call.hpp input_gate_t).
bool verify_batch_gate_ok(uint64_t nbatches, uint64_t nitems);
// The comb phase's verdict per vote, as launch_batch_signers fills it and a batch_call_t's
// `votes` hands it on.
struct batch_votes_t {
  const uint32_t* state;   // one word per vote of the call (nw_strict.hpp kVotePass ...)
  const uint32_t* list;    // the votes whose state is not kVotePass, dense, in any order
  const uint32_t* count;   // their number (device)
  uint32_t* live;          // nitems words: a slice's chunks that hold a listed vote
  uint32_t* nlive;         // their number (device; cleared per slice)
};
// The one launcher: every field of the call is described in nw_batch_call.hpp, and
// batch_call_check there says which combinations are refused (hipErrorInvalidValue).
hipError_t launch_verify_batch(const batch_call_t& call, hipStream_t stream);
// verify_batch over per-vote messages of any length (dalek's verify_batch(messages, signatures,
// public_keys)): vote i's message is msg_lengths[i] bytes at data + msg_offsets[i] (device
// arrays, one entry per vote of the call, any alignment). call.digests is the caller's k plane
// (32 bytes per vote: a job's own device buffer, the nw_dev_* caller's workspace; not a shared
// per-device buffer, so it needs no lease). Unless `hashed` (the caller has already run
// launch_strict_hram on `stream`: the comb phase reads the plane first), k_strict_hram runs once
// over all votes of the call, before the slice loop; then launch_verify_batch runs over the
// plane (kplane), with call.skip_group_ok / votes as launch_batch_signers left them
// (skip_per_group = 1, skip_pip). A lone large batch runs k_pip_points_k, k_pip_sort and the
// separate tail kernels, as a skip_pip call does.
hipError_t launch_verify_batch_msgs(batch_call_t call, const uint8_t* data,
                                    const uint64_t* msg_offsets, const uint64_t* msg_lengths,
                                    bool hashed, hipStream_t stream);
// Signature::verify_batch under the registered signers (nw_kernels.hip, DESIGN.md 5 "Round 12"):
// every vote of the call through the comb check under its registered key (sg.n != 0; bcomb: the
// device's B comb), the parities in batched inversions; *batch_ok_out (in scratch, nbatches words)
// = 1 for a batch all of whose votes passed, which is then Ok under verify_batch for every
// coefficient set, 0 otherwise. Follow with launch_verify_batch(skip_group_ok = *batch_ok_out,
// skip_per_group = 1, skip_pip = true). scratch: batch_signers_bytes(nbatches, nitems) of
// device memory; counters: 6 device words of 64 bits (set here): votes passed, votes not passed,
// batches settled, batches sent on, then the votes of the batches sent on that are left out
// of their sums and those that run in them. offsets: nbatches + 1 values from 0.
// votes_out (optional): filled with the per-vote states and the dense list of the votes that
// did not pass (one atomic per workgroup; the count stays on the device), to be handed to
// launch_verify_batch, which then leaves the passed votes out. Null (NW_BATCH_SIGNERS_VOTES=0,
// batch_signers_votes()): no list, every vote of a batch sent on runs, counter 4 stays 0.
// batch_signers_min_votes(): the call size from which the path is taken (NW_BATCH_SIGNERS_MIN_VOTES,
// default 1; NW_BATCH_SIGNERS=0: never), read per call.
// kplane: `digests` is the call's k plane (launch_strict_hram), one row per vote, and the comb
// check reads vote i's k from row i (k_batch_signers_k) instead of hashing its batch's digest.
constexpr int kBatchSignersCounters = 6;
size_t batch_signers_bytes(uint64_t nbatches, uint64_t nitems);
uint64_t batch_signers_min_votes();
bool batch_signers_votes();
hipError_t launch_batch_signers(const uint32_t* digests, const uint64_t* offsets, uint64_t nbatches,
                                const uint32_t* pks, const uint32_t* sigs, uint64_t nitems,
                                const strict_signers_t& sg, const struct ge_niels_pad* bcomb,
                                void* scratch, unsigned long long* counters,
                                const uint32_t** batch_ok_out, hipStream_t stream,
                                batch_votes_t* votes_out = nullptr, bool kplane = false);

// Certificate::verify vote batches merged over groups of certificates (nw_batch.hip):
// cert_group_size() = certificates per group, 0 when the merge does not apply;
// group scratch = cert_groups_bytes(ncert); the batch workspace is the same as
// launch_verify_batch's (batch_workspace_bytes(ncert, nvotes)). *group_ok_out points into
// group_ws (1 per group that passed).
struct ge;
// target_votes: votes per merged group (0 = do not merge); NW_CERT_GROUP_VOTES overrides.
uint64_t cert_group_size(const uint64_t* host_cvo, uint64_t ncert, uint64_t nkeys,
                         bool injected_z, uint64_t target_votes);
bool cert_group_env_fixed();
// fb (host-mapped, 8 words): [0] sequence, [1] groups, [2] groups that failed, [3] tag,
// [4] counted certificates, [5] counted certificates whose vote batch failed. cnt: 3 device
// words, zero before the first call (left zero). Launch after the per-certificate
// verify_batch (batch_st final); group_ok may be null (K = 0).
hipError_t launch_group_feedback(const uint32_t* group_ok, uint64_t ncert, uint64_t K,
                                 uint32_t tag, const int32_t* batch_st, const int32_t* pre1,
                                 const int32_t* pre2, const int32_t* hdr_st, uint32_t* cnt,
                                 uint32_t* fb, hipStream_t stream);
size_t cert_groups_bytes(uint64_t ncert);
const ge* key_tables_base(const ge_niels_pad* tabs, uint64_t nkeys, const keyspec& ks);
hipError_t launch_cert_groups(const uint32_t* cert_digest, const uint64_t* cvo,
                              const uint64_t* host_cvo, uint64_t ncert, const uint32_t* pks,
                              const uint32_t* sigs, uint64_t nvotes, const z_key_t& zkey,
                              void* batch_ws, void* group_ws, const int32_t* pre1,
                              const int32_t* pre2, const int32_t* hdr_st,
                              const key_tables_t& keys, const ge* key_base, uint32_t nkeys,
                              uint64_t K, uint32_t** group_ok_out, hipStream_t stream);
// Small groups: K certificates per keyed Straus check, then the per-certificate
// verify_batch of the certificates of failed groups from the same per-vote items. Writes
// status / fail_index for every certificate (in place of launch_verify_batch);
// cert_sgroup_size() picks K for an estimated fraction p_cert of certificates whose votes
// fail (NW_CERT_SMALL_K fixes it), 0 when merging does not apply; *beats_per_cert: the
// cost model prefers these groups to every certificate's own ladder. keys.vote_key required.
uint64_t cert_sgroup_size(const uint64_t* host_cvo, uint64_t ncert, uint64_t nkeys,
                          bool injected_z, double p_cert, bool* beats_per_cert);
hipError_t launch_cert_sgroups(const uint32_t* cert_digest, const uint64_t* cvo,
                               const uint64_t* host_cvo, uint64_t ncert, const uint32_t* pks,
                               const uint32_t* sigs, uint64_t nvotes, const z_key_t& zkey,
                               void* batch_ws, void* group_ws, const int32_t* pre1,
                               const int32_t* pre2, const int32_t* hdr_st,
                               const key_tables_t& keys, uint32_t nkeys, uint64_t K,
                               double p_cert, int32_t* status, uint64_t* fail_index,
                               uint32_t** group_ok_out, hipStream_t stream);
// Keyed vote checks (nw_kernels.hip): every undecided certificate's votes
// through the keyed comb one by one, R compared in compressed form (no decompression; the
// x parities in batched inversions); cert_ok[c] = 1 when all of them pass (then
// verify_batch is Ok too), 0 otherwise. Follow with launch_verify_batch(skip_group_ok =
// cert_ok, skip_per_group = 1). vote_cert: certificate of each vote (k_cert_prepare);
// cert_ok: ncert words; scratch: >= votes_keyed_fixed_bytes() + 64 x
// votes_keyed_bytes_per_vote() bytes (slices of the votes go through it, each checked in
// key-major order). keys.vote_key required; nkeys = committee size.
// hdr_st may be NULL (votes checked concurrently with the headers); then follow the join
// with launch_cert_ok_headers so header-failed certificates skip their verify_batch.
hipError_t launch_cert_ok_headers(const int32_t* hdr_st, uint64_t ncert, uint32_t* cert_ok,
                                  hipStream_t stream);
size_t votes_keyed_bytes_per_vote();
size_t votes_keyed_fixed_bytes();
hipError_t launch_votes_keyed(const uint32_t* cert_digest, const uint64_t* cvo, uint64_t ncert,
                              const uint32_t* vote_cert, const uint32_t* pks,
                              const uint32_t* sigs, uint64_t nvotes, const int32_t* pre1,
                              const int32_t* pre2, const int32_t* hdr_st,
                              const key_tables_t& keys, uint32_t nkeys, uint32_t* cert_ok,
                              void* scratch, size_t scratch_bytes, hipStream_t stream);

// ---- primary messages (nw_cert.hip) ----------------------------------------------------
struct cert_committee_t {
  uint64_t nauth;
  const uint32_t* pks;              // nauth x 8 words, sorted by bytes
  const uint32_t* stakes;
  const uint64_t* worker_offsets;   // nauth + 1
  const uint32_t* worker_ids;
};

struct cert_stream_t {
  uint64_t n;
  const uint8_t* header_bytes;
  const uint64_t* header_offsets;   // n + 1
  const uint32_t* payload_counts;
  const uint32_t* ids;              // n x 8 words
  const uint64_t* vote_offsets;     // n + 1
  const uint32_t* vote_pks;         // nvotes x 8 words
};

hipError_t launch_cert_prepare(const cert_committee_t& com, const cert_stream_t& cs,
                               int headers_only, const uint32_t* hdr_digest, uint32_t* authors,
                               uint32_t* cert_digest, int32_t* pre1, int32_t* pre2,
                               uint64_t* idx1, uint64_t* idx2, uint32_t* vote_key,
                               uint32_t* author_key, uint32_t* vote_cert, uint64_t nvotes,
                               hipStream_t stream);
hipError_t launch_cert_finalize(uint64_t n, int headers_only, const int32_t* pre1,
                                const int32_t* pre2, const uint64_t* idx1, const uint64_t* idx2,
                                const int32_t* hdr_status, const int32_t* batch_status,
                                const uint64_t* batch_index, int32_t* status, uint64_t* index,
                                hipStream_t stream);
hipError_t launch_vote_prepare(const cert_committee_t& com, uint64_t n, const uint32_t* ids,
                               const uint64_t* rounds, const uint32_t* origins,
                               const uint32_t* authors, uint32_t* digests, int32_t* pre,
                               uint32_t* author_key, hipStream_t stream);
hipError_t launch_vote_finalize(uint64_t n, const int32_t* pre, const int32_t* sig_status,
                                int32_t* status, hipStream_t stream);

// ---- wire ingest: bincode frames -> structure-of-arrays (nw_wire.hip, nw_wiredec.hpp) ----
// frames: the frame bytes as aligned words (readable up to the next multiple of 4 past
// total_bytes), offsets: n + 1 byte offsets from 0 to total_bytes. The scan writes one
// wd::rec_t per frame (kind = wd::kOverCap for a frame longer than max_frame, which it does
// not walk); the emit writes the rows of every frame whose wd::dst_t names a slot, group
// lanes (16 or 64) per frame. The canon kernel (after the scan) writes one wd::canon_t per
// frame and, for every non-canonical Header / Certificate frame of at most wd::kCanonMax
// entries, its order list into `order` (order_cap = wd::canon_list_words(total_bytes) words),
// with 64 or 256 lanes per workgroup and LDS for lds_entries (1..wd::kCanonMax) entries, no
// fewer than any scanned frame of the call can hold (a frame of len bytes: len / 32); with cans != nullptr the emit writes those frames' rows
// through their lists.
namespace wd {
struct rec_t;
struct dst_t;
struct out_t;
struct canon_t;
}  // namespace wd
hipError_t launch_wire_scan(const uint32_t* frames, const uint64_t* offsets, uint64_t n,
                            uint64_t total_bytes, uint64_t max_frame, wd::rec_t* recs,
                            hipStream_t stream);
hipError_t launch_wire_emit(const uint32_t* frames, const uint64_t* offsets, uint64_t n,
                            uint64_t total_bytes, const wd::rec_t* recs, const wd::dst_t* dsts,
                            const wd::canon_t* cans, const uint32_t* order, uint64_t order_cap,
                            const wd::out_t& out, uint32_t group, hipStream_t stream);
hipError_t launch_wire_canon(const uint32_t* frames, const uint64_t* offsets, uint64_t n,
                             uint64_t total_bytes, const wd::rec_t* recs, wd::canon_t* cans,
                             uint32_t* order, uint64_t order_cap, uint32_t lanes,
                             uint32_t lds_entries, hipStream_t stream);

// ---- small jobs in one launch (nw_small.hip) --------------------------------------------
// Header / Vote / Certificate checks of a small job (the aggregation service's latency
// path): one launch, no copies (inputs read from and outputs written to the job's pinned
// host buffer), only read access to the committee's key tables and the B comb.
enum : uint32_t { kSmallCerts = 0, kSmallHeaders = 1, kSmallVotes = 2 };
// One signature ("slot"): message m, j = 0 for the header signature (or the vote's own), j >= 1
// for certificate vote j - 1; v = global index of that vote (for j = 0 of a certificate: of
// its first vote); cnt = slots of the message (1 + votes for a certificate, else 1).
struct small_slot_t {
  uint32_t m, j, v, cnt;
};
struct small_msg_info_t {
  int32_t p1, p2;   // pre-signature verdicts: header level (-1 = genesis) / quorum
  uint64_t x1, x2;
};
struct small_job_t {
  uint32_t kind;           // kSmall*
  uint32_t slots_per_wg;   // S: 4, 8, 16, 32 or 64
  uint64_t nmsg, nslots;
  cert_committee_t com;    // 1..256 authorities
  // headers / certificates (nw_certificates layout; header offsets rebased to 0)
  const uint8_t* hb;
  const uint64_t* ho;
  const uint32_t* pc;
  const uint32_t* ids;     // also the votes' header ids
  const uint32_t* hsig;
  const uint32_t* vpk;     // certificate votes
  const uint32_t* vsig;
  const uint32_t* z16;     // optional injected batch coefficients (per vote)
  // votes (Vote::verify)
  const uint64_t* rounds;
  const uint32_t* origins;
  const uint32_t* authors;
  const uint32_t* sigs;
  const small_slot_t* slots;
  // device: the committee's key tables (built for exactly these keys) and the B comb
  const struct ge_niels_pad* ktabs;
  const uint32_t* kok;
  keyspec ks;              // the key tables' layout
  const struct ge_niels_pad* bcomb;
  uint32_t zkey[8];        // ChaCha20 key of the batch coefficients when z16 is null
  // device scratch: message info and slot records of messages spanning workgroups, and
  // the per-message arrival counters (zero before the launch, left zero after it)
  small_msg_info_t* minfo;
  uint32_t* srec;
  uint32_t* mcount;
  // outputs (pinned host memory)
  int32_t* status;
  uint64_t* index;
  uint64_t* stamps;        // diagnostics (NW_SMALL_STAMPS): 8 phase times per workgroup, or null
  // optional (pinned): workgroup w stores done_seq into done_flags[w] (system scope) after
  // its last status / index write, so the host sees the job finished before its completion
  // event (a workgroup that stored nothing just leaves the host waiting for the event)
  uint32_t* done_flags;
  uint32_t done_seq;
};
hipError_t upload_small_consts();
hipError_t launch_small(const small_job_t& job, hipStream_t stream);
// The keyed comb's B tables of the current device (built on first use).
hipError_t bcomb_table(const struct ge_niels_pad** out);

}  // namespace nw
