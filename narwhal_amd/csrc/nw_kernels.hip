// nw_kernels.hip — gfx950 kernels for Narwhal's crypto hot path.
//
//   k_sha512_digest32     Digest(Sha512(m)[..32]) for many messages, one lane per message
//                         (worker/src/processor.rs:38, primary/src/messages.rs:70-84 ...).
//   k_verify_strict       crypto::Signature::verify (crypto/src/lib.rs:200-204), one lane per
//                         signature: decompress A and R, small-order tests, k = H(R||A||M)
//                         mod l, half-size scalars, [v]R + [u]A + [w]B == 0 by one joint
//                         signed-window ladder (A and R tables in per-lane scratch, w in
//                         24-bit windows over device-built global tables), identity test.
//   k_btab_build          the strict kernel's B tables, once per device.
//   (crypto::Signature::verify_batch lives in nw_batch.hip.)
//
// Everything here is integer VALU work; no MFMA (modular arithmetic is not a contraction).
#include "nw_kernels.h"
#include "nw_point.hpp"
#include "nw_scalar.hpp"
#include "nw_sha512.hpp"
#include "nw_ladder.hpp"
#include "nw_consts.hpp"

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <type_traits>
#include <vector>

namespace nw {

struct dev_consts {
  curve_consts k;
  ge_niels btab[129];   // j * B, j = 0..128, affine niels (signed 8-bit windows)
  strict_consts sk;     // nw_strict.hpp: small-order y values
  ge_niels b128[129];   // j * 2^128 B
};

__constant__ dev_consts g_consts;

static constexpr int BT_WORDS = 129 * 30;

// ---------------------------------------------------------------------------------------
// Small helpers
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t bswap32(uint32_t x) { return __builtin_bswap32(x); }

// Copy a 129-entry niels table from constant memory into LDS (all threads of the block).
__device__ __forceinline__ void load_table(ge_niels* dst_tab, const ge_niels* src_tab) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(src_tab);
  uint32_t* dst = reinterpret_cast<uint32_t*>(dst_tab);
  for (int i = threadIdx.x; i < BT_WORDS; i += blockDim.x) dst[i] = src[i];
}
__device__ __forceinline__ void load_btab(ge_niels* s_btab) { load_table(s_btab, g_consts.btab); }

// Maximum of a per-lane value 0 <= w < 128 over the ACTIVE lanes of the wave (wave-uniform
// result), bit by bit with ballots, so it is exact inside divergent code too (a lane shuffle
// would read inactive lanes' stale registers).
struct WaveMax {
  __device__ int operator()(int w) const {
    int r = 0;
#pragma unroll
    for (int b = 6; b >= 0; --b) {
      const int c = r | (1 << b);
      if (__ballot(w >= c) != 0) r = c;
    }
    return r;
  }
};

// SHA-512 of the 96-byte R || A || M (one block) -> 16 LE words of the digest.
__device__ __forceinline__ void hram96(uint32_t x[16], const uint32_t R[8], const uint32_t A[8],
                                       const uint32_t M[8]) {
  uint64_t w[16], st[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    w[i] = ((uint64_t)bswap32(R[2 * i]) << 32) | bswap32(R[2 * i + 1]);
    w[4 + i] = ((uint64_t)bswap32(A[2 * i]) << 32) | bswap32(A[2 * i + 1]);
    w[8 + i] = ((uint64_t)bswap32(M[2 * i]) << 32) | bswap32(M[2 * i + 1]);
  }
  w[12] = 0x8000000000000000ULL;
  w[13] = 0;
  w[14] = 0;
  w[15] = 96 * 8;
  sha512_init(st);
  sha512_compress(st, w);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    x[2 * i] = bswap32((uint32_t)(st[i] >> 32));
    x[2 * i + 1] = bswap32((uint32_t)st[i]);
  }
}

// ---------------------------------------------------------------------------------------
// SHA-512 digests of many messages (lane per message)
// ---------------------------------------------------------------------------------------
// One lane per message (sha512_digest32_lane, nw_sha512.hpp: full blocks double-buffered,
// so a lone wave per SIMD -- config 3: 65,536 messages = 1,024 waves -- does not stall on
// each block's HBM latency).
__global__ __launch_bounds__(256) void k_sha512_digest32(const uint8_t* __restrict__ data,
                                                         const uint64_t* __restrict__ offsets,
                                                         const uint64_t* __restrict__ lengths,
                                                         uint64_t n, uint32_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint8_t* msg = data + offsets[i];
  const uint64_t len = lengths ? lengths[i] : offsets[i + 1] - offsets[i];
  sha512_digest32_lane(msg, len, out + 8 * i);
}

// ---------------------------------------------------------------------------------------
// Strict verification
// ---------------------------------------------------------------------------------------

// Makes p opaque to the optimiser: a load through the result is not merged with an earlier
// load of the same address, so inputs are re-fetched where they are needed instead of
// being kept live (and spilled) across the decompression.
template <class T>
__device__ __forceinline__ const T* opaque_ptr(const T* p) {
  asm volatile("" : "+v"(p));
  return p;
}

// strict_verify_core's inputs for item i, fetched from global memory when needed.
struct strict_src_global {
  static constexpr bool kPre = false;
  static constexpr bool kScalars = false;
  static constexpr bool kSharedA = false;
  const uint32_t* pk;    // 8 words
  const uint32_t* sig;   // 16 words: R || s
  const uint32_t* msg;   // 8 words
  __device__ void A(uint32_t w[8]) const {
    const uint32_t* p = opaque_ptr(pk);
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = p[j];
  }
  __device__ void R(uint32_t w[8]) const {
    const uint32_t* p = opaque_ptr(sig);
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = p[j];
  }
  __device__ void S(uint32_t w[8]) const {
    const uint32_t* p = opaque_ptr(sig);
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = p[8 + j];
  }
  // k = SHA-512(R || A || M) mod l over the raw bytes
  __device__ void K(uint32_t kw[8]) const {
    uint32_t Aw[8], Rw[8], Mw[8], hx[16];
    A(Aw);
    R(Rw);
    const uint32_t* m = opaque_ptr(msg);
#pragma unroll
    for (int j = 0; j < 8; ++j) Mw[j] = m[j];
    hram96(hx, Rw, Aw, Mw);
    sc k;
    sc_reduce512(k, hx);
#pragma unroll
    for (int j = 0; j < 8; ++j) kw[j] = k.w[j];
  }
};

// The same inputs with k already computed (launch_verify_strict_msgs: k_strict_hram hashed
// R || A || M for a message of any length and reduced it): K() is eight loads from the item's
// row of the k plane, no hash and no reduction. The instances over this source are kernels of
// their own (k_strict_triage_k, k_strict_keyed_hot_k, k_strict_keyed_signers_k), so those over
// strict_src_global keep their code objects.
struct strict_src_plane {
  static constexpr bool kPre = false;
  static constexpr bool kScalars = false;
  static constexpr bool kSharedA = false;
  const uint32_t* pk;    // 8 words
  const uint32_t* sig;   // 16 words: R || s
  const uint32_t* k;     // 8 words: SHA-512(R || A || M) mod l
  __device__ void A(uint32_t w[8]) const {
    const uint32_t* p = opaque_ptr(pk);
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = p[j];
  }
  __device__ void R(uint32_t w[8]) const {
    const uint32_t* p = opaque_ptr(sig);
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = p[j];
  }
  __device__ void S(uint32_t w[8]) const {
    const uint32_t* p = opaque_ptr(sig);
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = p[8 + j];
  }
  __device__ void K(uint32_t kw[8]) const {
    const uint32_t* p = opaque_ptr(k);
#pragma unroll
    for (int j = 0; j < 8; ++j) kw[j] = p[j];
  }
};

// k of every item of a strict launch over messages of any length (launch_verify_strict_msgs):
// one lane per item hashes R || A || M (sha512_hram_lane, nw_sha512.hpp: message i is lengths[i]
// bytes at data + offsets[i], any alignment), reduces mod l and writes the 8 words at
// kplane + 8 i, the shape of the 32-byte launch's digests array. A wave runs as long as its
// longest message.
__global__ __launch_bounds__(256) void k_strict_hram(const uint8_t* __restrict__ data,
                                                     const uint64_t* __restrict__ offsets,
                                                     const uint64_t* __restrict__ lengths,
                                                     const uint32_t* __restrict__ pks,
                                                     const uint32_t* __restrict__ sigs, uint64_t n,
                                                     uint32_t* __restrict__ kplane) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t Rw[8], Aw[8], hx[16];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    Rw[j] = sigs[16 * i + j];
    Aw[j] = pks[8 * i + j];
  }
  sha512_hram_lane(hx, Rw, Aw, data + offsets[i], lengths[i]);
  sc k;
  sc_reduce512(k, hx);
#pragma unroll
  for (int j = 0; j < 8; ++j) kplane[8 * i + j] = k.w[j];
}

// The same inputs with A's and R's x already decompressed (k_strict_triage): x limb k of
// point pt (0 = A, 1 = R) of survivor q at xs[(10 pt + k) cap + q]. y is the encoding's own
// (fe_frombytes), Z = 1, T = x y: exactly the point ge_frombytes returned. The same pass also
// ran the scalar phase (nw_strict.hpp strict_triage_scalars) and stored the ladder's digit
// word t at plane 20 + t and vneg | W << 1 at plane 41. A survivor whose key has a slot in the
// slice's key set (nw_strict.hpp keyset_probe) has kMetaSharedA set in plane 41 and the slot
// number in plane 0 (A's x limb 0; its limbs 1..9 are not written): its table j * A is
// ktabs[8 slot ..], built once by k_strict_keys_build.
constexpr uint64_t kTriagePlanes = 20 + kStrictDigitWords + 1;
struct strict_src_pre : strict_src_global {
  static constexpr bool kPre = true;
  static constexpr bool kScalars = true;
  static constexpr bool kSharedA = true;
  const uint32_t* xs;
  uint64_t cap, q;
  const ge_cached_pk* ktabs;
  __device__ uint32_t shared_slot() const {
    const uint32_t* x = opaque_ptr(xs);
    const uint32_t meta = x[(uint64_t)(20 + kStrictDigitWords) * cap + q];
    return (meta & kMetaSharedA) ? x[q] : kNoSlot;
  }
  __device__ const void* shared_tabs() const { return ktabs; }
  __device__ bool point(int pt, ge& P) const {
    uint32_t w[8];
    if (pt) R(w); else A(w);
    fe_frombytes(P.Y, w);
    const uint32_t* x = opaque_ptr(xs) + (uint64_t)(10 * pt) * cap + q;
#pragma unroll
    for (int k = 0; k < 10; ++k) P.X.v[k] = x[(uint64_t)k * cap];
    fe_1(P.Z);
    fe_mul(P.T, P.X, P.Y);
    return true;
  }
  __device__ uint32_t digit_word(int t) const {
    return opaque_ptr(xs)[(uint64_t)(20 + t) * cap + q];
  }
  __device__ uint32_t scalar_meta() const {
    return digit_word(kStrictDigitWords) & ~kMetaSharedA;
  }
};

// Limb planes of the pending votes of a slice: X' limb k at planes[k S + i], Z' limb k at
// planes[(10 + k) S + i] (coalesced in both kernels); state[i] = kVote* of vote v0 + i.
struct vote_planes_t {
  uint32_t* planes;
  uint32_t* state;
  uint64_t S;
  const uint32_t* perm;   // slice position -> slice vote (key-major order), or nullptr
};

#ifndef NW_KEYED_WAVES
#define NW_KEYED_WAVES 1
#endif
// The strict ladder's LDS prefetcher (nw_strict.hpp pf_none for the contract): one
// 128-byte slot per lane (8 chunks of 16 B, chunk k of lane l at s_pf[k][l]: the lanes of a
// wave write and read 16 consecutive bytes each, conflict-free), 32 KB per 256-thread block.
// Every entry is one 128-byte line: a B-table entry (affine niels, ge_niels_pad) or a
// per-lane entry packed to 128 B (ge_cached_pk; unpacked here).
#ifndef NW_STRICT_PF
#define NW_STRICT_PF 1
#endif
// (The keyed comb checks through the same slots measured slower)
#if NW_STRICT_PF && NW_BWIN != 8
// The ladder's digit words (u, |v|, w recoded: 21 per lane) live in LDS too, 21 KB per block:
// read with a wave-uniform index once per addition, they were otherwise a scratch array (a
// dependent scratch load per addition; scratch 272 -> 180 B per lane, +0.2 % in the same
// process, profiles/r05w). 53 KB per block: three blocks per CU fit the 160 KB.
__shared__ uint4 s_pf[8][256];
__shared__ uint32_t s_dig[21][256];
struct pf_lds {
  static constexpr bool enabled = true;
  static constexpr bool lds_digits = true;
  uint32_t wave;   // wave index in the block (uniform)
  __device__ void dput(int k, uint32_t v) const { s_dig[k][threadIdx.x] = v; }
  __device__ uint32_t dget(int k) const { return s_dig[k][threadIdx.x]; }
  __device__ void issue(const void* src, int chunks) const {
    const uint4* g = static_cast<const uint4*>(src);
    __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): this lane's last slot read is done
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (k < chunks) __builtin_amdgcn_global_load_lds(g + k, &s_pf[k][wave * 64], 16, 0, 0);
  }
  __device__ void get(ge_cached& e, bool niels) const {
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): the DMA into LDS has landed
    asm volatile("" ::: "memory");
    const uint32_t l = threadIdx.x;
    uint32_t p[32];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const uint4 v = s_pf[k][l];
      p[4 * k] = v.x; p[4 * k + 1] = v.y; p[4 * k + 2] = v.z; p[4 * k + 3] = v.w;
    }
    if (niels) {   // y+x, y-x, xy2d (-> YpX, YmX, T2d; Z2 unused)
#pragma unroll
      for (int i = 0; i < 10; ++i) {
        e.YpX.v[i] = p[i];
        e.YmX.v[i] = p[10 + i];
        e.T2d.v[i] = p[20 + i];
      }
      return;
    }
    fe_unpack(e.YpX, p);
    fe_unpack(e.YmX, p + 8);
    fe_unpack(e.Z2, p + 16);
    fe_unpack(e.T2d, p + 24);
  }
  // A packed per-lane entry read as -entry when neg (NW_PF_SWAP): Y+X and Y-X trade places
  // through the LDS address (chunks 0-1 <-> 2-3), so the caller negates only 2dT.
  __device__ void get_signed(ge_cached& e, bool neg) const {
    __builtin_amdgcn_s_waitcnt(0x0F70);
    asm volatile("" ::: "memory");
    const uint32_t l = threadIdx.x;
    const uint32_t a = neg ? 2u : 0u;
    uint32_t p[32];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const uint4 v = s_pf[k < 4 ? (k ^ a) : k][l];
      p[4 * k] = v.x; p[4 * k + 1] = v.y; p[4 * k + 2] = v.z; p[4 * k + 3] = v.w;
    }
    fe_unpack(e.YpX, p);
    fe_unpack(e.YmX, p + 8);
    fe_unpack(e.Z2, p + 16);
    fe_unpack(e.T2d, p + 24);
  }
};
#endif

// Persistent: the grid covers the resident waves once and strides over the items, so the
// per-lane tables j*A, j*R live in a fixed workspace (16 packed entries x 128 B per lane slot,
// lane-contiguous: a lookup reads one 128-byte line per lane instead of 40 scattered dwords).
#ifndef NW_STRICT_WAVES
#define NW_STRICT_WAVES 3
#endif
// KEYED = false: arbitrary keys only, every item through the half-size ladder (config 4,
// nw_verify_strict_many): the instance carries neither the keyed comb branch nor the list
// mode, so their registers and code do not weigh on the ladder. KEYED = true: committee
// keys take the keyed comb, and `list` (the keyed fast path's leftovers) is honoured.
template <bool KEYED>
__global__ __launch_bounds__(256, NW_STRICT_WAVES) void k_verify_strict(const uint32_t* __restrict__ msgs,
                                                       uint32_t msg_stride_words,
                                                       const uint32_t* __restrict__ pks,
                                                       const uint32_t* __restrict__ sigs,
                                                       uint64_t n, int32_t* __restrict__ status,
                                                       uint64_t* __restrict__ bitmap,
                                                       ge_cached_pk* __restrict__ tabs,
                                                       key_tables_t keys,
                                                       const ge_niels_pad* __restrict__ btw,
                                                       const ge_niels_pad* __restrict__ bcomb,
                                                       const uint32_t* __restrict__ list,
                                                       const uint32_t* __restrict__ list_count) {
  // list mode (keyed fast path's leftovers): items list[0 .. *list_count), no bitmap words
  if (!KEYED) list = nullptr;
  if (list) n = *list_count;
#if NW_BWIN == 8
  __shared__ ge_niels s_btab[129];
  __shared__ ge_niels s_b128[129];
  load_table(s_btab, g_consts.btab);
  load_table(s_b128, g_consts.b128);
  __syncthreads();
  const btab_pair bt{s_btab, s_b128};
  (void)btw;
#else
  const btab_wide bt{btw, bdigits<NW_BWIN>::ENTRIES};
#endif
  ge_cached_pk* tabA = tabs + 16 * ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x);
  ge_cached_pk* tabR = tabA + 8;
#pragma unroll 1
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n;
       base += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t gi = base + threadIdx.x;
    const bool active = gi < n;
    const uint64_t i = list ? list[active ? gi : n - 1] : active ? gi : n - 1;
    const strict_src_global src{pks + 8 * i, sigs + 16 * i, msgs + (uint64_t)msg_stride_words * i};
    const uint32_t kk = KEYED && keys.vote_key ? keys.vote_key[i] : kNoKey;
    const ge_niels_pad* keytab = kk != kNoKey ? keys.tabs + keys.ks.tab * (uint64_t)kk : nullptr;
    // committee keys: [s]B - [k]A from comb tables, no ladder; others: the half-size ladder
    int st;
    if (KEYED && keytab) {
      st = strict_keyed_comb(src, g_consts.sk, bcomb_wide{bcomb}, keytab_wide{keytab, keys.ks},
                             keys.ok[kk]);
    } else {
#if NW_STRICT_PF && NW_BWIN != 8
      st = strict_verify_core<NW_BWIN>(src, g_consts.sk, bt, tabA, tabR, WaveMax{},
                                       pf_lds{(uint32_t)__builtin_amdgcn_readfirstlane(
                                           threadIdx.x >> 6)});
#else
      st = strict_verify_core<NW_BWIN>(src, g_consts.sk, bt, tabA, tabR, WaveMax{});
#endif
    }
    if (active) status[i] = st;
    if (list) continue;
    const uint64_t mask = __ballot(active && st == NW_OK);
    if ((threadIdx.x & 63) == 0 && gi < n) bitmap[gi >> 6] = mask;
  }
}

// ---- config 4's strict verification in two passes (NW_STRICT_TRIAGE, default on) ----
// Every check before the equation (s's high bits and canonical form, A's and R's
// decompression and small order) needs only the two square roots, ~15 % of a verification;
// an item that fails one of them (7 of the 12 invalid classes of the mixed corpus, ~6.5 % of
// its items) still ran the whole ladder in k_verify_strict, whose lanes all take the same
// path. k_strict_triage runs the checks for a slice of items, one lane per item, writes the
// verdict of every item that fails one (same order as strict_verify_core: crypto/src/lib.rs
// 201-202, then dalek's verify_strict), and appends the others to a list with the x of A and
// R; k_verify_strict_pre runs strict_verify_core on the list, loading those points instead
// of decompressing them (strict_src_pre). Statuses are the same codes for every item.
// With the comb path's to-do list an entry may say that the comb check decided its item
// (kTodoDecided: R' = [s]B - [k]A is not the point R encodes): the triage then settles it, as
// NW_ERR_EQUATION unless its own checks reject it, and the list never sees it.
#ifndef NW_TRIAGE_WAVES
#define NW_TRIAGE_WAVES 4   // waves per SIMD (129 VGPRs unbounded: 3)
#endif
// (the kernel's text: nw_strict_triage_kernel.hpp, once per source of an item's inputs)
#define NW_TRIAGE_KERNEL k_strict_triage
#define NW_TRIAGE_SRC strict_src_global
#include "nw_strict_triage_kernel.hpp"
// The triage of a launch over messages of any length: k comes from the k plane (msgs, stride 8).
#define NW_TRIAGE_KERNEL k_strict_triage_k
#define NW_TRIAGE_SRC strict_src_plane
#include "nw_strict_triage_kernel.hpp"

// ---- the slice's key set (nw_strict.hpp keyset_probe / keyset_build) ----
struct keyset_atomics {
  __device__ uint32_t load(const uint32_t* p) const {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ uint32_t cas(uint32_t* p, uint32_t expect, uint32_t val) const {
    return atomicCAS(p, expect, val);
  }
  __device__ void inc(uint32_t* p) const { atomicAdd(p, 1u); }
};
// One lane per item of the slice: keyslot[j] = the slot of item j's key, or kNoSlot.
// with[block & (kKeyStatLanes - 1)] += the block's items with a slot (diagnostics: one atomic
// per block, spread over kKeyStatLanes addresses).
__global__ __launch_bounds__(256) void k_strict_keys_probe(
    const uint32_t* __restrict__ pks, uint64_t i0, uint64_t ns, uint32_t* slots, uint32_t cap,
    uint32_t limit, uint32_t* nkeys, uint32_t* __restrict__ keyslot,
    unsigned long long* __restrict__ with_ctr, uint32_t* __restrict__ uses) {
  __shared__ uint32_t s_with[4];
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = j < ns;
  uint32_t slot = kNoSlot;
  if (active) {
    slot = keyset_probe(slots, cap, limit, nkeys, pks, i0, (uint32_t)j, keyset_atomics{});
    keyslot[j] = slot;
    // uses[slot] += kCombSample for the items of a fixed 1-in-kCombSample sample: an estimate
    // of the slice's items under that key (the comb path's hot-key choice; nw_strict.hpp)
    if (uses && slot != kNoSlot && comb_sampled((uint32_t)j)) atomicAdd(uses + slot, kCombSample);
  }
  const uint64_t m = __ballot(slot != kNoSlot);
  if ((threadIdx.x & 63u) == 0) s_with[threadIdx.x >> 6] = (uint32_t)__builtin_popcountll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t with = s_with[0] + s_with[1] + s_with[2] + s_with[3];
    if (with) atomicAdd(with_ctr + (blockIdx.x & (kKeyStatLanes - 1)), (unsigned long long)with);
  }
}
// One lane per slot: an owned slot's flags and table. stats[0] += owned slots.
__global__ __launch_bounds__(256) void k_strict_keys_build(
    const uint32_t* __restrict__ pks, uint64_t i0, const uint32_t* __restrict__ slots,
    uint32_t cap, uint32_t* __restrict__ kflags, ge_cached_pk* __restrict__ ktabs,
    unsigned long long* __restrict__ stats) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  const bool owned = s < cap && slots[s] != 0;
  const uint64_t m = __ballot(owned);
  if (m == 0) return;
  if ((threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(m))
    atomicAdd(stats, (unsigned long long)__builtin_popcountll(m));
  if (owned) keyset_build(slots, s, pks, i0, g_consts.sk, kflags, ktabs);
}

// The slice's keys that are registered signers (nw_strict.hpp signers_lookup): one lane per slot
// of the slice's key set; an owned slot whose key decodes and is not small looks its owner's 32
// bytes up in the registry: match[slot] = the registry row or kNoKey. The work is per distinct
// key, not per item. *nlive += matched slots (the slice's comb kernels run when it is not 0),
// *matched += the same (diagnostics), one atomic each per wave that has any.
__global__ __launch_bounds__(256) void k_strict_signers_match(
    const uint32_t* __restrict__ pks, uint64_t i0, const uint32_t* __restrict__ slots, uint32_t cap,
    const uint32_t* __restrict__ kflags, signers_view sv, uint32_t* __restrict__ match,
    uint32_t* __restrict__ nlive, unsigned long long* __restrict__ matched) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t row = kNoKey;
  if (s < cap) {
    const uint32_t owner = slots[s];
    if (owner != 0 && comb_key_hot(0, 0, kflags[s])) {
      uint32_t w[8];
      const uint32_t* key = pks + 8 * (i0 + (owner - 1));
#pragma unroll
      for (int t = 0; t < 8; ++t) w[t] = key[t];
      row = signers_lookup(sv, w);
    }
    match[s] = row;
  }
  const uint64_t m = __ballot(row != kNoKey);
  if (m && (threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(m)) {
    const uint32_t c = (uint32_t)__builtin_popcountll(m);
    atomicAdd(nlive, c);
    atomicAdd(matched, (unsigned long long)c);
  }
}

// The slice's hot keys (comb_key_hot): one lane per slot; a hot slot takes the next dense index
// while there are fewer than hot_cap (which slots win may differ from run to run, no status
// does): hotidx[slot] = its index or kNoKey, hotrow[index] = the owner item's row in the slice.
// *nhot may end above hot_cap; its readers clamp it. cstats[0] += hot keys taken.
// With registered signers (match != nullptr, k_strict_signers_match's plane): one index space,
// the nreg registry rows first, then the call-local tables. A matched slot gets its registry
// row and takes no ticket (no table is built for it, whatever its use count); any other slot
// that turns hot gets nreg + its ticket and adds one to *nlive.
__global__ __launch_bounds__(256) void k_strict_comb_select(
    const uint32_t* __restrict__ slots, uint32_t cap, const uint32_t* __restrict__ kflags,
    const uint32_t* __restrict__ uses, uint32_t min_uses, uint32_t hot_cap,
    uint32_t* __restrict__ nhot, uint32_t* __restrict__ hotidx, uint32_t* __restrict__ hotrow,
    unsigned long long* __restrict__ cstats, const uint32_t* __restrict__ match, uint32_t nreg,
    uint32_t* __restrict__ nlive) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= cap) return;
  uint32_t h = match ? match[s] : kNoKey;
  const uint32_t owner = slots[s];
  if (h == kNoKey && owner != 0 && hot_cap != 0 && comb_key_hot(uses[s], min_uses, kflags[s])) {
    const uint32_t t = atomicAdd(nhot, 1u);
    if (t < hot_cap) {
      h = nreg + t;
      hotrow[t] = owner - 1;
      atomicAdd(cstats, 1ull);
      if (nlive) atomicAdd(nlive, 1u);
    }
  }
  hotidx[s] = h;
}

// Key-major order of the slice (nw_strict_keymajor.hpp): a counting sort of its items by the
// index the comb kernels use, hotidx[keyslot[i]], in groups of 2^shift indices; every item
// without a live key goes to the last bin. k_km_hist / k_km_scan / k_km_scatter follow the
// votes' k_vk_* below: blocks take contiguous chunks of kKmChunk items, count them in an LDS
// histogram and touch global memory with ONE atomic per (block, bin used) and pass; positions
// inside a block's range of a bin come from LDS cursors. 12.5M items under 4,096 keys: 763
// blocks x ~513 bins, 0.39M atomics per pass over 513 addresses (a block per 256 items, or a
// bin per key, would be millions on as many addresses as the votes' 4.9 ms pass had).
// The counts are exact and the sort's own (uses[] is a sampled estimate). All three exit when
// the slice has fewer than min_live live keys, a word every kernel of the slice reads alike.
struct km_keys_t {
  const uint32_t* keyslot;   // item -> slot of the slice's key set, or kNoSlot
  const uint32_t* hotidx;    // slot -> key index, or kNoKey (k_strict_comb_select)
  const uint32_t* nhot;      // call-local tables taken; may end above hot_cap
  const uint32_t* live;      // the slice's live keys (comb_block_t nhot or nlive)
  uint32_t nreg, hot_cap, min_live;
};
__device__ __forceinline__ uint32_t km_space(const km_keys_t& k) {
  const uint32_t nhot = *k.nhot;
  return k.nreg + (nhot < k.hot_cap ? nhot : k.hot_cap);
}
__device__ __forceinline__ uint32_t km_item_bin(const km_keys_t& k, uint64_t i, uint32_t space,
                                                uint32_t shift, uint32_t* slot_out) {
  const uint32_t slot = k.keyslot[i];
  *slot_out = slot;
  return km_bin(slot != kNoSlot ? k.hotidx[slot] : kNoKey, space, shift);
}
__global__ __launch_bounds__(256) void k_km_hist(uint64_t ns, km_keys_t k,
                                                 uint32_t* __restrict__ gh) {
  __shared__ uint32_t h[kKmBins];
  if (*k.live < k.min_live) return;
  const uint32_t space = km_space(k), shift = km_shift(space);
  for (uint32_t b = threadIdx.x; b < kKmBins; b += blockDim.x) h[b] = 0;
  __syncthreads();
  const uint64_t c0 = (uint64_t)blockIdx.x * kKmChunk;
  const uint64_t c1 = c0 + kKmChunk < ns ? c0 + kKmChunk : ns;
  uint32_t slot;
  for (uint64_t i = c0 + threadIdx.x; i < c1; i += blockDim.x)
    atomicAdd(&h[km_item_bin(k, i, space, shift, &slot)], 1u);
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < kKmBins; b += blockDim.x)
    if (h[b]) atomicAdd(&gh[b], h[b]);
}
// One block of kKmBins lanes: cursor[b] = the first position of bin b (an exclusive scan of
// the histogram, which is left zero for the next slice), *npos = the last bin's, the
// launch's counters.
__global__ __launch_bounds__(kKmBins) void k_km_scan(uint32_t* __restrict__ gh,
                                                     uint32_t* __restrict__ cursor,
                                                     km_block_t* __restrict__ blk,
                                                     const uint32_t* __restrict__ live,
                                                     uint32_t min_live) {
  __shared__ uint32_t s[kKmBins];
  __shared__ uint32_t s_used[kKmBins / 64];
  if (*live < min_live) return;
  const uint32_t b = threadIdx.x;
  const uint32_t c = gh[b];
  gh[b] = 0;
  s[b] = c;
  const uint64_t used = __ballot(c != 0 && b != kKmBins - 1);
  if ((b & 63u) == 0) s_used[b >> 6] = (uint32_t)__builtin_popcountll(used);
  __syncthreads();
  for (uint32_t d = 1; d < kKmBins; d <<= 1) {   // Hillis-Steele, inclusive
    const uint32_t v = b >= d ? s[b - d] : 0u;
    __syncthreads();
    s[b] += v;
    __syncthreads();
  }
  cursor[b] = s[b] - c;
  if (b == kKmBins - 1) {
    const uint32_t npos = s[b] - c;
    uint32_t bins = 0;
    for (uint32_t w = 0; w < kKmBins / 64; ++w) bins += s_used[w];
    blk->npos = npos;
    blk->placed += npos;   // one lane of one block per slice: no atomic needed
    blk->bins += bins;
    blk->slices += 1;
  }
}
// Same chunks: count again, reserve the block's range in every bin it uses (one atomic each),
// then hand out positions inside the ranges with LDS cursors. perm[p] = the item at position
// p, pslot[p] = its slot. The positions of all bins together are exactly 0 .. ns - 1.
__global__ __launch_bounds__(256) void k_km_scatter(uint64_t ns, km_keys_t k,
                                                    uint32_t* __restrict__ cursor,
                                                    uint32_t* __restrict__ perm,
                                                    uint32_t* __restrict__ pslot) {
  __shared__ uint32_t h[kKmBins];
  if (*k.live < k.min_live) return;
  const uint32_t space = km_space(k), shift = km_shift(space);
  for (uint32_t b = threadIdx.x; b < kKmBins; b += blockDim.x) h[b] = 0;
  __syncthreads();
  const uint64_t c0 = (uint64_t)blockIdx.x * kKmChunk;
  const uint64_t c1 = c0 + kKmChunk < ns ? c0 + kKmChunk : ns;
  uint32_t slot;
  for (uint64_t i = c0 + threadIdx.x; i < c1; i += blockDim.x)
    atomicAdd(&h[km_item_bin(k, i, space, shift, &slot)], 1u);
  __syncthreads();
  for (uint32_t x = threadIdx.x; x < kKmBins; x += blockDim.x)
    if (h[x]) h[x] = atomicAdd(&cursor[x], h[x]);   // this block's range in bin x
  __syncthreads();
  for (uint64_t i = c0 + threadIdx.x; i < c1; i += blockDim.x) {
    const uint32_t b = km_item_bin(k, i, space, shift, &slot);
    const uint32_t p = atomicAdd(&h[b], 1u);
    if (p < ns) {   // always: the ranges partition 0 .. ns - 1 (a guard, not a path)
      perm[p] = (uint32_t)i;
      pslot[p] = slot;
    }
  }
}

// The list's items (persistent, as k_verify_strict): strict_verify_core on the points
// k_strict_triage decompressed; *count is read on the device.
__global__ __launch_bounds__(256, NW_STRICT_WAVES) void k_verify_strict_pre(
    const uint32_t* __restrict__ msgs, uint32_t msg_stride_words, const uint32_t* __restrict__ pks,
    const uint32_t* __restrict__ sigs, uint64_t i0, const uint32_t* __restrict__ list,
    const uint32_t* __restrict__ count, const uint32_t* __restrict__ xs, uint64_t cap,
    int32_t* __restrict__ status, ge_cached_pk* __restrict__ tabs,
    const ge_niels_pad* __restrict__ btw, const ge_cached_pk* __restrict__ ktabs,
    unsigned long long* __restrict__ ladder_total) {
  const uint64_t n = *count;
  // *ladder_total (optional) += the slice's items that come here (diagnostics, kept over a
  // launch's slices: one atomic per slice)
  if (ladder_total && n && blockIdx.x == 0 && threadIdx.x == 0)
    atomicAdd(ladder_total, (unsigned long long)n);
#if NW_BWIN == 8
  __shared__ ge_niels s_btab[129];
  __shared__ ge_niels s_b128[129];
  load_table(s_btab, g_consts.btab);
  load_table(s_b128, g_consts.b128);
  __syncthreads();
  const btab_pair bt{s_btab, s_b128};
  (void)btw;
#else
  const btab_wide bt{btw, bdigits<NW_BWIN>::ENTRIES};
#endif
  ge_cached_pk* tabA = tabs + 16 * ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x);
  ge_cached_pk* tabR = tabA + 8;
#pragma unroll 1
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n;
       base += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t q0 = base + threadIdx.x;
    const bool active = q0 < n;
    const uint64_t q = active ? q0 : n - 1;
    const uint64_t i = i0 + list[q];
    const strict_src_pre src{{pks + 8 * i, sigs + 16 * i, msgs + (uint64_t)msg_stride_words * i},
                             xs, cap, q, ktabs};
#if NW_STRICT_PF && NW_BWIN != 8
    const int st = strict_verify_core<NW_BWIN>(src, g_consts.sk, bt, tabA, tabR, WaveMax{},
                                               pf_lds{(uint32_t)__builtin_amdgcn_readfirstlane(
                                                   threadIdx.x >> 6)});
#else
    const int st = strict_verify_core<NW_BWIN>(src, g_consts.sk, bt, tabA, tabR, WaveMax{});
#endif
    if (active) status[i] = st;
  }
}

// Keyed fast path of launch_verify_strict (committee-key signers: Header::verify authors,
// Vote::verify voters). k_strict_keyed runs the certificate votes' check (nw_strict.hpp
// keyed_vote_check: [s]B - [k]A from the comb tables, compared with R in compressed form,
// no square root) on every keyed item of a slice; a pass IS dalek's verify_strict Ok
// (status 0), everything else — fails, non-committee signers, parity mismatches found by
// k_strict_keyed_inv — is appended to a list (k_strict_keyed_list) and verified by
// k_verify_strict in list mode, which names the exact failing check (status 1..7). With
// honest streams the list is short, so the ~265-squaring decompression of R is skipped
// for almost every signature.
// HOT = false: a committee's tables, item i's key is vote_key[vk0 + i]. HOT = true: the call's
// hot keys (launch_verify_strict's comb path): vote_key[vk0 + i] is the item's slot in the
// slice's key set and slotmap[slot] its key's index in the call's 8-bit tables (or kNoKey),
// valid below *nlive; *checked += items with a key. There the state also tells the two kinds of
// failure apart (kVoteFail / kVoteDecided, strict_keyed_item below): k_strict_todo_list hands a
// decided item's verdict to the triage, which settles it without the ladder (DESIGN.md 5
// "Round 11"); the committee branch lists both kinds alike for k_verify_strict. NW_COMB_WAVES: waves per SIMD of the HOT
// instance (1 to 4 measured alike on config 4; the LDS prefetcher measured 4 % slower there,
// as it did for committee tables: DESIGN.md 5 "Round 9").
#ifndef NW_COMB_WAVES
#define NW_COMB_WAVES 1
#endif
// Key-major order of the HOT instances' lanes (nw_strict_keymajor.hpp; the order itself is
// vote_planes_t's perm, null for a launch in item order): what a lane needs besides it.
struct km_order_t {
  const uint32_t* pslot;   // position -> the item's slot in the slice's key set
  const uint32_t* slots;   // the key set: slot -> its owner's row in the slice + 1
  uint32_t min_live;       // the slice is sorted when it has at least this many live keys
};
// The device's part of the decision, taken alike by the sort kernels and by every kernel that
// reads the order, from words that are final once k_strict_comb_select has run.
__device__ __forceinline__ bool km_sorted(const uint32_t* perm, uint32_t live, uint32_t min_live) {
  return perm != nullptr && live >= min_live;
}
__device__ __forceinline__ bool km_sorted(const uint32_t* perm, uint32_t live,
                                          const km_order_t& km) {
  return km_sorted(perm, live, km.min_live);
}
__device__ __forceinline__ const km_order_t* km_ptr() { return nullptr; }
__device__ __forceinline__ const km_order_t* km_ptr(const km_order_t& km) { return &km; }

// The check of slice item i (global item gi) under the key whose comb tables are `tab` and whose
// flag word is *okword (tab == nullptr: the item has no key here) and what it leaves behind:
// status 0 for a pass, X' / Z' in the planes for a pending parity, the state word: kVoteFail
// for an item without a key or one that left the check before the comb sum, kVoteDecided for
// one whose sum ran and gave Y' != y_R Z' (nw_strict.hpp keyed_vote_check_ex).
// i is the item's place in the planes (its slice index, or its position in key-major order);
// key_row the row of pks that holds its key's 32 bytes (gi, or the row of any item of the same
// slot of the key set, which compares all 32 bytes).
template <class Src = strict_src_global>
__device__ __forceinline__ void strict_keyed_item(
    const uint32_t* __restrict__ msgs, uint32_t msg_stride_words, const uint32_t* __restrict__ pks,
    const uint32_t* __restrict__ sigs, uint64_t gi, uint64_t i, int32_t* __restrict__ status,
    const ge_niels_pad* __restrict__ tab, const keyspec& ks, const uint32_t* __restrict__ okword,
    const ge_niels_pad* __restrict__ bcomb, const vote_planes_t& vp, uint64_t key_row) {
  uint32_t st = kVoteFail;
  if (tab) {
    const Src src{pks + 8 * key_row, sigs + 16 * gi, msgs + (uint64_t)msg_stride_words * gi};
    fe X, Z;
    st = keyed_vote_check_ex(src, g_consts.sk, bcomb_wide{bcomb}, keytab_wide{tab, ks}, *okword, X,
                             Z);
    if (st >= kVotePending) {
#pragma unroll
      for (int k = 0; k < 10; ++k) {
        vp.planes[(uint64_t)k * vp.S + i] = X.v[k];
        vp.planes[(uint64_t)(10 + k) * vp.S + i] = Z.v[k];
      }
    }
  }
  if (st == kVotePass) status[gi] = NW_OK;
  vp.state[i] = st;
}
// (k_strict_keyed's body over either source of an item's inputs: inlined into k_strict_keyed
// it compiles to the instructions the kernel had with the body written in it)
template <bool HOT, class Src>
__device__ __forceinline__ void strict_keyed_body(
    const uint32_t* __restrict__ msgs, uint32_t msg_stride_words, const uint32_t* __restrict__ pks,
    const uint32_t* __restrict__ sigs, uint64_t i0, uint64_t ns, int32_t* __restrict__ status,
    const key_tables_t& keys, const ge_niels_pad* __restrict__ bcomb, const vote_planes_t& vp,
    uint64_t vk0, const uint32_t* __restrict__ slotmap, const uint32_t* __restrict__ nlive,
    unsigned long long* __restrict__ checked, const km_order_t* km) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ns) return;
  if constexpr (HOT) {
    if (*nlive == 0) return;   // no hot key: the triage takes the whole slice
  }
  uint64_t gi = i0 + i, key_row = gi;
  uint32_t kk;
  if constexpr (HOT) {
    // lane i is position i of the key-major order (vp.perm, nw_strict_keymajor.hpp) when the
    // slice was sorted, else item i
    if (km_sorted(vp.perm, *nlive, *km)) {
      gi = i0 + vp.perm[i];
      kk = km->pslot[i];
      key_row = kk != kNoSlot ? i0 + (km->slots[kk] - 1) : gi;
    } else {
      kk = keys.vote_key[vk0 + i];
    }
    kk = kk != kNoSlot ? slotmap[kk] : kNoKey;
    if (kk != kNoKey && kk >= *nlive) kk = kNoKey;
    const uint64_t m = __ballot(kk != kNoKey);
    if (m && (threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(m))
      atomicAdd(checked, (unsigned long long)__builtin_popcountll(m));
  } else {
    kk = keys.vote_key[vk0 + i];
  }
  const bool has = kk != kNoKey;
  strict_keyed_item<Src>(msgs, msg_stride_words, pks, sigs, gi, i, status,
                         has ? keys.tabs + keys.ks.tab * (uint64_t)kk : nullptr, keys.ks,
                         keys.ok + (has ? kk : 0u), bcomb, vp, key_row);
}
// Km: nothing for the committee instance (HOT = false, whose arguments and code are those it
// had before the key-major order), one km_order_t for the HOT one.
template <bool HOT, class... Km>
__global__ __launch_bounds__(256, HOT ? NW_COMB_WAVES : NW_KEYED_WAVES) void k_strict_keyed(
    const uint32_t* __restrict__ msgs, uint32_t msg_stride_words, const uint32_t* __restrict__ pks,
    const uint32_t* __restrict__ sigs, uint64_t i0, uint64_t ns, int32_t* __restrict__ status,
    key_tables_t keys, const ge_niels_pad* __restrict__ bcomb, vote_planes_t vp,
    uint64_t vk0, const uint32_t* __restrict__ slotmap, const uint32_t* __restrict__ nlive,
    unsigned long long* __restrict__ checked, Km... km) {
  static_assert(sizeof...(Km) == (HOT ? 1 : 0), "the HOT instance takes the order, no other does");
  strict_keyed_body<HOT, strict_src_global>(msgs, msg_stride_words, pks, sigs, i0, ns, status,
                                            keys, bcomb, vp, vk0, slotmap, nlive, checked,
                                            km_ptr(km...));
}
// k_strict_keyed<true> of a launch over messages of any length: k from the k plane (msgs).
__global__ __launch_bounds__(256, NW_COMB_WAVES) void k_strict_keyed_hot_k(
    const uint32_t* __restrict__ msgs, uint32_t msg_stride_words, const uint32_t* __restrict__ pks,
    const uint32_t* __restrict__ sigs, uint64_t i0, uint64_t ns, int32_t* __restrict__ status,
    key_tables_t keys, const ge_niels_pad* __restrict__ bcomb, vote_planes_t vp,
    uint64_t vk0, const uint32_t* __restrict__ slotmap, const uint32_t* __restrict__ nlive,
    unsigned long long* __restrict__ checked, km_order_t km) {
  strict_keyed_body<true, strict_src_plane>(msgs, msg_stride_words, pks, sigs, i0, ns, status,
                                            keys, bcomb, vp, vk0, slotmap, nlive, checked, &km);
}
// The HOT instance over one index space (k_strict_comb_select with registered signers): index
// kk < nreg is row kk of the registry's tables (rtabs, rok), any other one call-local table
// kk - nreg of `keys`, valid below *nhot. A kernel of its own, so that k_strict_keyed<true>
// keeps its code object; it counts nothing (k_strict_signers_count does, afterwards).
// *nlive == 0: no hot key and no registered key in the slice, the triage takes all of it.
template <class Src>
__device__ __forceinline__ void strict_keyed_signers_body(
    const uint32_t* __restrict__ msgs, uint32_t msg_stride_words, const uint32_t* __restrict__ pks,
    const uint32_t* __restrict__ sigs, uint64_t i0, uint64_t ns, int32_t* __restrict__ status,
    const key_tables_t& keys, const ge_niels_pad* __restrict__ bcomb, const vote_planes_t& vp,
    const uint32_t* __restrict__ slotmap, const uint32_t* __restrict__ nhot,
    const uint32_t* __restrict__ nlive, const ge_niels_pad* __restrict__ rtabs,
    const uint32_t* __restrict__ rok, uint32_t nreg, const km_order_t& km) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ns || *nlive == 0) return;
  uint64_t gi = i0 + i, key_row = gi;
  uint32_t kk;
  if (km_sorted(vp.perm, *nlive, km)) {   // lane i is position i of the key-major order
    gi = i0 + vp.perm[i];
    kk = km.pslot[i];
    key_row = kk != kNoSlot ? i0 + (km.slots[kk] - 1) : gi;
  } else {
    kk = keys.vote_key[i];
  }
  kk = kk != kNoSlot ? slotmap[kk] : kNoKey;
  const bool reg = kk < nreg;
  if (kk != kNoKey && !reg) {
    kk -= nreg;
    if (kk >= *nhot) kk = kNoKey;
  }
  const bool has = kk != kNoKey;
  strict_keyed_item<Src>(msgs, msg_stride_words, pks, sigs, gi, i, status,
                         has ? (reg ? rtabs : keys.tabs) + keys.ks.tab * (uint64_t)kk : nullptr,
                         keys.ks, (reg ? rok : keys.ok) + (has ? kk : 0u), bcomb, vp, key_row);
}
__global__ __launch_bounds__(256, NW_COMB_WAVES) void k_strict_keyed_signers(
    const uint32_t* __restrict__ msgs, uint32_t msg_stride_words, const uint32_t* __restrict__ pks,
    const uint32_t* __restrict__ sigs, uint64_t i0, uint64_t ns, int32_t* __restrict__ status,
    key_tables_t keys, const ge_niels_pad* __restrict__ bcomb, vote_planes_t vp,
    const uint32_t* __restrict__ slotmap, const uint32_t* __restrict__ nhot,
    const uint32_t* __restrict__ nlive, const ge_niels_pad* __restrict__ rtabs,
    const uint32_t* __restrict__ rok, uint32_t nreg, km_order_t km) {
  strict_keyed_signers_body<strict_src_global>(msgs, msg_stride_words, pks, sigs, i0, ns, status,
                                               keys, bcomb, vp, slotmap, nhot, nlive, rtabs, rok,
                                               nreg, km);
}
// The same of a launch over messages of any length: k from the k plane (msgs).
__global__ __launch_bounds__(256, NW_COMB_WAVES) void k_strict_keyed_signers_k(
    const uint32_t* __restrict__ msgs, uint32_t msg_stride_words, const uint32_t* __restrict__ pks,
    const uint32_t* __restrict__ sigs, uint64_t i0, uint64_t ns, int32_t* __restrict__ status,
    key_tables_t keys, const ge_niels_pad* __restrict__ bcomb, vote_planes_t vp,
    const uint32_t* __restrict__ slotmap, const uint32_t* __restrict__ nhot,
    const uint32_t* __restrict__ nlive, const ge_niels_pad* __restrict__ rtabs,
    const uint32_t* __restrict__ rok, uint32_t nreg, km_order_t km) {
  strict_keyed_signers_body<strict_src_plane>(msgs, msg_stride_words, pks, sigs, i0, ns, status,
                                              keys, bcomb, vp, slotmap, nhot, nlive, rtabs, rok,
                                              nreg, km);
}

// Parity of the pending items (Montgomery's trick per strided chunk, as k_votes_keyed_inv).
// keyed_inv_chunk: the chunk of one lane, shared with k_batch_signers_inv; done(i, match)
// settles pending item i. k_strict_keyed_inv: a match is status 0, a mismatch goes to the list
// as kVoteDecided (R' = -decode(R): the equation fails whatever else the full verification
// would look at).
template <class Done>
__device__ __forceinline__ void keyed_inv_chunk(uint64_t lane, uint64_t ns, uint64_t nchunks,
                                                const vote_planes_t& vp, const Done& done) {
  auto load = [&](fe& f, int base, uint64_t i) {
#pragma unroll
    for (int k = 0; k < 10; ++k) f.v[k] = vp.planes[(uint64_t)(base + k) * vp.S + i];
  };
  fe acc;
  fe_1(acc);
  uint64_t last = ~0ull;
#pragma unroll 1
  for (uint64_t i = lane; i < ns; i += nchunks) {
    if (vp.state[i] < kVotePending) continue;
    fe X, Z, W;
    load(X, 0, i);
    load(Z, 10, i);
    fe_mul(W, X, acc);
#pragma unroll
    for (int k = 0; k < 10; ++k) vp.planes[(uint64_t)k * vp.S + i] = W.v[k];
    fe_mul(acc, acc, Z);
    last = i;
  }
  if (last == ~0ull) return;
  fe inv;
  fe_invert(inv, acc);
#pragma unroll 1
  for (uint64_t i = last;; i -= nchunks) {
    const uint32_t st = vp.state[i];
    if (st >= kVotePending) {
      fe W, Z, x;
      load(W, 0, i);
      load(Z, 10, i);
      fe_mul(x, W, inv);
      done(i, fe_isnegative(x) == (st & 1));
      fe_mul(inv, inv, Z);
    }
    if (i < nchunks) break;
  }
}
__global__ __launch_bounds__(256) void k_strict_keyed_inv(uint64_t i0, uint64_t ns,
                                                          uint64_t nchunks,
                                                          int32_t* __restrict__ status,
                                                          vote_planes_t vp,
                                                          const uint32_t* __restrict__ nlive,
                                                          uint32_t km_min) {
  // nlive (optional): nothing to do when *nlive == 0 (k_strict_keyed<true> wrote no state)
  const uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= nchunks || (nlive && *nlive == 0)) return;
  // the planes and the state are in position space when the slice was sorted: position i holds
  // item perm[i]
  const uint32_t* const perm = nlive && km_sorted(vp.perm, *nlive, km_min) ? vp.perm : nullptr;
  keyed_inv_chunk(lane, ns, nchunks, vp, [&](uint64_t i, bool match) {
    if (match) status[i0 + (perm ? perm[i] : i)] = NW_OK;
    else vp.state[i] = comb_parity_state(false);
  });
}

// Failed / unkeyed items of the slice -> list (one atomic per wave).
__global__ __launch_bounds__(256) void k_strict_keyed_list(uint64_t i0, uint64_t ns,
                                                           const uint32_t* __restrict__ state,
                                                           uint32_t* __restrict__ list,
                                                           uint32_t* __restrict__ count) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool f = i < ns && vote_failed(state[i]);   // kVoteDecided is listed like kVoteFail
  const uint64_t m = __ballot(f);
  if (m == 0) return;
  const uint32_t lane = threadIdx.x & 63;
  uint32_t base = 0;
  if (lane == (uint32_t)(__ffsll((unsigned long long)m) - 1))
    base = atomicAdd(count, (uint32_t)__popcll(m));
  base = (uint32_t)__shfl((int)base, __ffsll((unsigned long long)m) - 1);
  if (f) list[base + (uint32_t)__popcll(m & ((1ull << lane) - 1))] = (uint32_t)(i0 + i);
}

// The same for the comb path's to-do list (slice-relative items, in no particular order): a
// block takes kTodoPer x 256 consecutive items and appends its failed ones with ONE atomic
// (a slice of 12.5M items with ~10 % of them failed: one atomic per wave was ~195 k
// same-address atomics, 4.6 ms).
// Both kinds of failure are listed. The triage cannot read an item's state (plane 20 at the
// item's index: it overwrites planes 0-20+ at the list positions of other items while it runs),
// so the entry carries it: bit 31 (comb_todo_entry) for kVoteDecided when `decide` is set
// (NW_STRICT_COMB_DECIDE, default on; off: every entry is plain, the sequence of rounds 9-10).
constexpr uint32_t kTodoPer = 16;
__global__ __launch_bounds__(256) void k_strict_todo_list(uint64_t ns,
                                                          const uint32_t* __restrict__ state,
                                                          uint32_t* __restrict__ list,
                                                          uint32_t* __restrict__ count,
                                                          const uint32_t* __restrict__ nlive,
                                                          uint32_t decide,
                                                          const uint32_t* __restrict__ perm,
                                                          uint32_t km_min) {
  __shared__ uint32_t s_wave[4];
  __shared__ uint32_t s_base;
  if (*nlive == 0) return;   // no hot key, no state: the triage takes the whole slice
  // a sorted slice: the state is per position, the entry names the item there
  if (!km_sorted(perm, *nlive, km_min)) perm = nullptr;
  const uint64_t b0 = (uint64_t)blockIdx.x * (256 * kTodoPer);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  // round r: items b0 + 256 r + threadIdx.x; this wave's failed items of all rounds, counted
  // (dmasks: those of them that are kVoteDecided)
  uint64_t masks[kTodoPer], dmasks[kTodoPer];
  uint32_t mine = 0;
#pragma unroll
  for (uint32_t r = 0; r < kTodoPer; ++r) {
    const uint64_t i = b0 + 256 * r + threadIdx.x;
    const uint32_t st = i < ns ? state[i] : kVotePass;
    masks[r] = __ballot(vote_failed(st));
    dmasks[r] = __ballot(st == kVoteDecided);
    mine += (uint32_t)__builtin_popcountll(masks[r]);
  }
  if (lane == 0) s_wave[wave] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t tot = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    s_base = tot ? atomicAdd(count, tot) : 0u;
  }
  __syncthreads();
  uint32_t pos = s_base;
  for (uint32_t w = 0; w < wave; ++w) pos += s_wave[w];
#pragma unroll
  for (uint32_t r = 0; r < kTodoPer; ++r) {
    const uint64_t m = masks[r];
    if ((m >> lane) & 1ull) {
      const uint32_t p = (uint32_t)(b0 + 256 * r + threadIdx.x);
      list[pos + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull))] =
          comb_todo_entry(perm ? perm[p] : p,
                          ((dmasks[r] >> lane) & 1ull) ? kVoteDecided : kVoteFail, decide != 0);
    }
    pos += (uint32_t)__builtin_popcountll(m);
  }
}

// Diagnostics of a slice that ran k_strict_keyed_signers, after k_strict_keyed_inv (an item the
// comb passed is any checked item whose state is neither kVoteFail nor kVoteDecided): ctr[c][lane] += the block's
// items c = 0 checked, 1 checked under a registered key, 2 passed under one. A block takes
// kTodoPer x 256 consecutive items and adds each of its sums with ONE atomic, spread over
// kCombStatLanes addresses.
__global__ __launch_bounds__(256) void k_strict_signers_count(
    uint64_t ns, const uint32_t* __restrict__ keyslot, const uint32_t* __restrict__ slotmap,
    const uint32_t* __restrict__ nhot, const uint32_t* __restrict__ nlive, uint32_t nreg,
    const uint32_t* __restrict__ state, unsigned long long* __restrict__ ctr,
    const uint32_t* __restrict__ perm, const uint32_t* __restrict__ pslot, uint32_t km_min) {
  __shared__ uint32_t s_sum[4][3];
  if (*nlive == 0) return;
  // a sorted slice: the state is per position, and so is the slot of the item there
  if (km_sorted(perm, *nlive, km_min)) keyslot = pslot;
  const uint64_t b0 = (uint64_t)blockIdx.x * (256 * kTodoPer);
  uint32_t mine[3] = {0, 0, 0};
#pragma unroll 1
  for (uint32_t r = 0; r < kTodoPer; ++r) {
    const uint64_t i = b0 + 256 * r + threadIdx.x;
    bool any = false, reg = false, pass = false;
    if (i < ns) {
      const uint32_t slot = keyslot[i];
      const uint32_t kk = slot != kNoSlot ? slotmap[slot] : kNoKey;
      reg = kk < nreg;
      any = reg || (kk != kNoKey && kk - nreg < *nhot);
      pass = reg && !vote_failed(state[i]);
    }
    mine[0] += (uint32_t)__builtin_popcountll(__ballot(any));
    mine[1] += (uint32_t)__builtin_popcountll(__ballot(reg));
    mine[2] += (uint32_t)__builtin_popcountll(__ballot(pass));
  }
  if ((threadIdx.x & 63u) == 0)
    for (int c = 0; c < 3; ++c) s_sum[threadIdx.x >> 6][c] = mine[c];
  __syncthreads();
  if (threadIdx.x < 3) {
    const uint32_t c = threadIdx.x;
    const uint32_t tot = s_sum[0][c] + s_sum[1][c] + s_sum[2][c] + s_sum[3][c];
    if (tot)
      atomicAdd(ctr + c * kCombStatLanes + (blockIdx.x & (kCombStatLanes - 1)),
                (unsigned long long)tot);
  }
}

// Verdict bitmap from the statuses (bit i set iff status[i] == 0), 64 items per wave.
__global__ __launch_bounds__(256) void k_status_bitmap(const int32_t* __restrict__ status,
                                                       uint64_t n, uint64_t* __restrict__ bitmap) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t m = __ballot(i < n && status[i] == NW_OK);
  if ((threadIdx.x & 63) == 0 && i < n) bitmap[i >> 6] = m;
}

// Certificate votes checked one by one with the keyed comb (Certificate::verify's
// Signature::verify_batch, messages.rs:212, without merging). A vote whose strict check
// passes satisfies R == [s]B - [k]A exactly, so its term of any random linear combination
// vanishes: a certificate all of whose votes pass is Ok under verify_batch too. Every other
// certificate keeps cert_ok = 0 and gets its own verify_batch (launch_verify_batch with
// skip_group_ok = cert_ok, one certificate per group), so statuses and fail indices are the
// per-certificate path's. Certificates already decided by an earlier check are left alone
// (their batch status is never read).
//
// R is never decompressed (nw_strict.hpp keyed_vote_check): R' = [s]B - [k]A is compared
// with R's encoding through Y' == y_R Z' and the parity of X'/Z'. The parity needs 1/Z':
// k_votes_keyed writes X', Z' of the votes that got that far into limb planes, and
// k_votes_keyed_inv inverts them in batches (Montgomery's trick, one lane per strided chunk
// of votes: 4 multiplications per vote and one inversion per chunk instead of the ~265
// squarings of a decompression per vote).
__global__ __launch_bounds__(256) void k_votes_keyed_init(const uint64_t* __restrict__ cvo,
                                                          uint64_t ncert,
                                                          uint32_t* __restrict__ cert_ok) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c < ncert) cert_ok[c] = cvo[c + 1] > cvo[c] ? 1u : 0u;   // no votes: its own batch
}


// Key-major order of a slice's votes (k_vk_hist / k_vk_scan / k_vk_scatter: a counting sort
// by committee key; the votes of already-decided certificates and non-members go to one
// last bin whose lanes do no comb work). With 16-bit key tables (67 MB per key) a wave whose
// lanes name ~64 different keys gathers from the whole committee's tables (6.7 GB at
// N = 100: HBM and TLB bound); sorted, the chip works on one or two keys' tables at a time,
// which stay in the last-level caches.
constexpr uint32_t kVkMaxBins = 1024;
constexpr uint32_t kVkSortMinKeys = 32;
__device__ __forceinline__ uint32_t vk_bin(const uint32_t* __restrict__ vote_cert,
                                           const uint32_t* __restrict__ vote_key, uint64_t v,
                                           const int32_t* __restrict__ pre1,
                                           const int32_t* __restrict__ pre2,
                                           const int32_t* __restrict__ hdr_st, uint32_t nkeys) {
  const uint32_t c = vote_cert[v];
  if (pre1[c] != 0 || (hdr_st && hdr_st[c] != 0) || pre2[c] != 0) return nkeys;
  const uint32_t k = vote_key[v];
  return k < nkeys ? k : nkeys;
}
// Blocks take contiguous chunks of kVkChunk votes: one global atomic per (block, bin), not
// per (256 votes, bin) — with ~100 bins per block the per-block form made the 26M global
// atomics of N = 100 serialize on 100 addresses (4.9 ms per pass).
constexpr uint32_t kVkChunk = 16384;
__global__ __launch_bounds__(256) void k_vk_hist(const uint32_t* __restrict__ vote_cert,
                                                 const uint32_t* __restrict__ vote_key,
                                                 uint64_t v0, uint64_t nv,
                                                 const int32_t* __restrict__ pre1,
                                                 const int32_t* __restrict__ pre2,
                                                 const int32_t* __restrict__ hdr_st,
                                                 uint32_t nkeys, uint32_t* __restrict__ gh) {
  __shared__ uint32_t h[kVkMaxBins];
  for (uint32_t b = threadIdx.x; b <= nkeys; b += blockDim.x) h[b] = 0;
  __syncthreads();
  const uint64_t c0 = (uint64_t)blockIdx.x * kVkChunk;
  const uint64_t c1 = c0 + kVkChunk < nv ? c0 + kVkChunk : nv;
  for (uint64_t i = c0 + threadIdx.x; i < c1; i += blockDim.x)
    atomicAdd(&h[vk_bin(vote_cert, vote_key, v0 + i, pre1, pre2, hdr_st, nkeys)], 1u);
  __syncthreads();
  for (uint32_t b = threadIdx.x; b <= nkeys; b += blockDim.x)
    if (h[b]) atomicAdd(&gh[b], h[b]);
}
__global__ __launch_bounds__(64) void k_vk_scan(uint32_t* __restrict__ gh, uint32_t nbins) {
  if (threadIdx.x != 0) return;
  uint32_t acc = 0;
  for (uint32_t b = 0; b < nbins; ++b) {
    const uint32_t c = gh[b];
    gh[b] = acc;
    acc += c;
  }
}
// Same chunks: count again, reserve the block's range in every bin (one atomic each), then
// hand out positions inside the ranges with LDS cursors.
__global__ __launch_bounds__(256) void k_vk_scatter(const uint32_t* __restrict__ vote_cert,
                                                    const uint32_t* __restrict__ vote_key,
                                                    uint64_t v0, uint64_t nv,
                                                    const int32_t* __restrict__ pre1,
                                                    const int32_t* __restrict__ pre2,
                                                    const int32_t* __restrict__ hdr_st,
                                                    uint32_t nkeys, uint32_t* __restrict__ cursor,
                                                    uint32_t* __restrict__ perm) {
  __shared__ uint32_t h[kVkMaxBins];
  for (uint32_t b = threadIdx.x; b <= nkeys; b += blockDim.x) h[b] = 0;
  __syncthreads();
  const uint64_t c0 = (uint64_t)blockIdx.x * kVkChunk;
  const uint64_t c1 = c0 + kVkChunk < nv ? c0 + kVkChunk : nv;
  for (uint64_t i = c0 + threadIdx.x; i < c1; i += blockDim.x)
    atomicAdd(&h[vk_bin(vote_cert, vote_key, v0 + i, pre1, pre2, hdr_st, nkeys)], 1u);
  __syncthreads();
  for (uint32_t x = threadIdx.x; x <= nkeys; x += blockDim.x)
    if (h[x]) h[x] = atomicAdd(&cursor[x], h[x]);   // this block's range in bin x
  __syncthreads();
  for (uint64_t i = c0 + threadIdx.x; i < c1; i += blockDim.x) {
    const uint32_t b = vk_bin(vote_cert, vote_key, v0 + i, pre1, pre2, hdr_st, nkeys);
    perm[atomicAdd(&h[b], 1u)] = (uint32_t)i;
  }
}

__global__ __launch_bounds__(256, NW_KEYED_WAVES) void k_votes_keyed(
    const uint32_t* __restrict__ cert_digest, const uint32_t* __restrict__ vote_cert,
    uint64_t v0, uint64_t nv, const uint32_t* __restrict__ pks,
    const uint32_t* __restrict__ sigs, const int32_t* __restrict__ pre1,
    const int32_t* __restrict__ pre2, const int32_t* __restrict__ hdr_st, key_tables_t keys,
    const ge_niels_pad* __restrict__ bcomb, uint32_t* __restrict__ cert_ok, vote_planes_t vp) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nv) return;
  const uint64_t v = v0 + (vp.perm ? vp.perm[i] : i);
  const uint32_t c = vote_cert[v];
  uint32_t st = kVotePass;
  if (pre1[c] == 0 && (!hdr_st || hdr_st[c] == 0) && pre2[c] == 0) {
    const uint32_t kk = keys.vote_key[v];
    if (kk == kNoKey) {   // not a committee key (cannot happen for an undecided certificate)
      st = kVoteFail;
    } else {
      const strict_src_global src{pks + 8 * v, sigs + 16 * v, cert_digest + 8 * (uint64_t)c};
      fe X, Z;
      st = keyed_vote_check(src, g_consts.sk, bcomb_wide{bcomb},
                            keytab_wide{keys.tabs + keys.ks.tab * (uint64_t)kk, keys.ks}, keys.ok[kk], X, Z);
      if (st >= kVotePending) {
#pragma unroll
        for (int k = 0; k < 10; ++k) {
          vp.planes[(uint64_t)k * vp.S + i] = X.v[k];
          vp.planes[(uint64_t)(10 + k) * vp.S + i] = Z.v[k];
        }
      }
    }
    if (st == kVoteFail) cert_ok[c] = 0;   // same value from every failing lane
  }
  vp.state[i] = st;
}

// After votes were checked concurrently with the headers (hdr_st not yet known to them):
// a certificate whose header failed is decided by its header, so it skips its own
// verify_batch (cert_ok = 1 is the skip flag there).
__global__ __launch_bounds__(256) void k_cert_ok_headers(const int32_t* __restrict__ hdr_st,
                                                         uint64_t ncert,
                                                         uint32_t* __restrict__ cert_ok) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c < ncert && hdr_st[c] != 0) cert_ok[c] = 1u;
}

// One lane per chunk {i = j * nchunks + lane}: Montgomery's trick over the chunk's pending
// votes. Forward: W_i = X'_i * (product of the earlier Z'), acc *= Z'_i (W_i over X'_i);
// one inversion of the product; backward: x_i = W_i * inv, inv *= Z'_i. A vote whose x
// parity differs from its sign bit fails its certificate.
__global__ __launch_bounds__(256) void k_votes_keyed_inv(const uint32_t* __restrict__ vote_cert,
                                                         uint64_t v0, uint64_t nv,
                                                         uint64_t nchunks,
                                                         uint32_t* __restrict__ cert_ok,
                                                         vote_planes_t vp) {
  const uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= nchunks) return;
  auto load = [&](fe& f, int base, uint64_t i) {
#pragma unroll
    for (int k = 0; k < 10; ++k) f.v[k] = vp.planes[(uint64_t)(base + k) * vp.S + i];
  };
  fe acc;
  fe_1(acc);
  uint64_t last = ~0ull;
#pragma unroll 1
  for (uint64_t i = lane; i < nv; i += nchunks) {
    if (vp.state[i] < kVotePending) continue;
    fe X, Z, W;
    load(X, 0, i);
    load(Z, 10, i);
    fe_mul(W, X, acc);
#pragma unroll
    for (int k = 0; k < 10; ++k) vp.planes[(uint64_t)k * vp.S + i] = W.v[k];
    fe_mul(acc, acc, Z);
    last = i;
  }
  if (last == ~0ull) return;
  fe inv;
  fe_invert(inv, acc);
#pragma unroll 1
  for (uint64_t i = last;; i -= nchunks) {
    const uint32_t st = vp.state[i];
    if (st >= kVotePending) {
      fe W, Z, x;
      load(W, 0, i);
      load(Z, 10, i);
      fe_mul(x, W, inv);
      if (fe_isnegative(x) != (st & 1))
        cert_ok[vote_cert[v0 + (vp.perm ? vp.perm[i] : i)]] = 0;
      fe_mul(inv, inv, Z);
    }
    if (i < nchunks) break;
  }
}

// ---- plain batches under the registered signers (DESIGN.md 5 "Round 12") ----
// Signature::verify_batch calls carry no committee, but their signers may be registered
// (strict_signers_t): every vote of the call takes the comb check under its registered key
// (nw_strict.hpp batch_signers_vote; k = SHA-512(R || A || digest of its batch)), the parities
// come from the strided inversion, and batch_ok[b] stays 1 only when every vote of batch b
// passed. launch_verify_batch then runs with batch_ok as its skip list. No kernel here waits
// for another block; a failing vote stores a plain 0 (the same value from every failing lane).
//   k_batch_signers_init   batch_ok[b] = 1 (an empty batch is settled), the four counters = 0
//   k_batch_signers        one lane per vote
//   k_batch_signers_inv    parities (keyed_inv_chunk); the state ends as kVotePass / kVoteFail
//   k_batch_signers_count  votes passed / not passed, batches settled / sent on: block sums,
//                          one atomic per counter and block; the votes of the batches sent on
//                          (counters 4 and 5); with `list`, the dense list of the votes that
//                          did not pass (a block's votes at a base from one atomic)
__device__ __forceinline__ uint64_t vote_batch(const uint64_t* __restrict__ offsets,
                                               uint64_t nbatches, uint64_t v) {
  uint64_t lo = 0, hi = nbatches;   // the last b with offsets[b] <= v (empty batches before it)
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) >> 1;
    if (offsets[mid] <= v) lo = mid; else hi = mid;
  }
  return lo;
}
__global__ __launch_bounds__(256) void k_batch_signers_init(uint64_t nbatches,
                                                            uint32_t* __restrict__ batch_ok,
                                                            unsigned long long* __restrict__ ctr,
                                                            uint32_t* __restrict__ nlist) {
  const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b < nbatches) batch_ok[b] = 1u;
  if (b < kBsCounters) ctr[b] = 0ull;
  if (b == 0 && nlist) *nlist = 0u;
}
// Src = strict_src_global: k from the digest of the vote's batch; strict_src_plane
// (k_batch_signers_k, the per-message entries): k from row i of the call's k plane.
template <class Src>
__device__ __forceinline__ void batch_signers_lane(
    const uint32_t* __restrict__ digests, const uint64_t* __restrict__ offsets, uint64_t nbatches,
    const uint32_t* __restrict__ pks, const uint32_t* __restrict__ sigs, uint64_t nv,
    const signers_view& sv, const uint32_t* __restrict__ rok, const uint32_t* __restrict__ rlam,
    const ge_niels_pad* __restrict__ rtabs, const ge_niels_pad* __restrict__ bcomb,
    uint32_t* __restrict__ batch_ok, const vote_planes_t& vp) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nv) return;
  const uint64_t b = vote_batch(offsets, nbatches, i);
  constexpr bool kPlane = std::is_same<Src, strict_src_plane>::value;
  const Src src{pks + 8 * i, sigs + 16 * i, digests + 8 * (kPlane ? i : b)};
  const keyspec ks = keyspec_for(8);
  fe X, Z;
  const uint32_t st = batch_signers_vote(
      src, g_consts.sk, bcomb_wide{bcomb}, sv, rok, rlam,
      [&](uint32_t row) { return keytab_wide{rtabs + ks.tab * (uint64_t)row, ks}; }, X, Z);
  if (st >= kVotePending) {
#pragma unroll
    for (int k = 0; k < 10; ++k) {
      vp.planes[(uint64_t)k * vp.S + i] = X.v[k];
      vp.planes[(uint64_t)(10 + k) * vp.S + i] = Z.v[k];
    }
  }
  if (st == kVoteFail) batch_ok[b] = 0u;
  vp.state[i] = st;
}
__global__ __launch_bounds__(256, NW_COMB_WAVES) void k_batch_signers(
    const uint32_t* __restrict__ digests, const uint64_t* __restrict__ offsets, uint64_t nbatches,
    const uint32_t* __restrict__ pks, const uint32_t* __restrict__ sigs, uint64_t nv,
    signers_view sv, const uint32_t* __restrict__ rok, const uint32_t* __restrict__ rlam,
    const ge_niels_pad* __restrict__ rtabs, const ge_niels_pad* __restrict__ bcomb,
    uint32_t* __restrict__ batch_ok, vote_planes_t vp) {
  batch_signers_lane<strict_src_global>(digests, offsets, nbatches, pks, sigs, nv, sv, rok, rlam,
                                        rtabs, bcomb, batch_ok, vp);
}
__global__ __launch_bounds__(256, NW_COMB_WAVES) void k_batch_signers_k(
    const uint32_t* __restrict__ kplane, const uint64_t* __restrict__ offsets, uint64_t nbatches,
    const uint32_t* __restrict__ pks, const uint32_t* __restrict__ sigs, uint64_t nv,
    signers_view sv, const uint32_t* __restrict__ rok, const uint32_t* __restrict__ rlam,
    const ge_niels_pad* __restrict__ rtabs, const ge_niels_pad* __restrict__ bcomb,
    uint32_t* __restrict__ batch_ok, vote_planes_t vp) {
  batch_signers_lane<strict_src_plane>(kplane, offsets, nbatches, pks, sigs, nv, sv, rok, rlam,
                                       rtabs, bcomb, batch_ok, vp);
}
__global__ __launch_bounds__(256) void k_batch_signers_inv(const uint64_t* __restrict__ offsets,
                                                           uint64_t nbatches, uint64_t nv,
                                                           uint64_t nchunks,
                                                           uint32_t* __restrict__ batch_ok,
                                                           vote_planes_t vp) {
  const uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= nchunks) return;
  keyed_inv_chunk(lane, nv, nchunks, vp, [&](uint64_t i, bool match) {
    vp.state[i] = match ? kVotePass : kVoteFail;
    if (!match) batch_ok[vote_batch(offsets, nbatches, i)] = 0u;
  });
}
__global__ __launch_bounds__(256) void k_batch_signers_count(
    uint64_t nv, const uint32_t* __restrict__ state, uint64_t nbatches,
    const uint32_t* __restrict__ batch_ok, const uint64_t* __restrict__ offsets,
    unsigned long long* __restrict__ ctr, uint32_t* __restrict__ list,
    uint32_t* __restrict__ nlist) {
  __shared__ uint32_t s_sum[4][4];
  __shared__ unsigned long long s_sent[4];
  __shared__ uint32_t s_base;
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool v = i < nv, b = i < nbatches;
  const bool pass = v && state[i] == kVotePass, okb = b && batch_ok[i] != 0;
  const bool is[4] = {pass, v && !pass, okb, b && !okb};   // kBsVotesPassed .. kBsSentOn
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint64_t mfail = __ballot(is[1]);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const uint32_t n = (uint32_t)__builtin_popcountll(__ballot(is[c]));
    if (lane == 0) s_sum[wv][c] = n;
  }
  // the votes of the batches sent on (a wave's sum by xor shuffles)
  unsigned long long sent = is[3] ? offsets[i + 1] - offsets[i] : 0ull;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sent += __shfl_xor(sent, o);
  if (lane == 0) s_sent[wv] = sent;
  __syncthreads();
  const uint32_t nfail = s_sum[0][1] + s_sum[1][1] + s_sum[2][1] + s_sum[3][1];
  if (threadIdx.x < 4) {
    const uint32_t c = threadIdx.x;
    const uint32_t tot = s_sum[0][c] + s_sum[1][c] + s_sum[2][c] + s_sum[3][c];
    if (tot) atomicAdd(ctr + c, (unsigned long long)tot);
  } else if (threadIdx.x == 4) {
    // a vote that did not pass belongs to a batch sent on, so with the list the votes left
    // out are those batches' votes less the ones not passed: the counter's final value is
    // that difference whatever the order of the blocks' additions (mod 2^64)
    const unsigned long long tot = s_sent[0] + s_sent[1] + s_sent[2] + s_sent[3];
    if (list) {
      if (tot != nfail) atomicAdd(ctr + kBsVotesLeftOut, tot - (unsigned long long)nfail);
      if (nfail) atomicAdd(ctr + kBsVotesRun, (unsigned long long)nfail);
    } else if (tot) {
      atomicAdd(ctr + kBsVotesRun, tot);
    }
  } else if (threadIdx.x == 5 && list && nfail) {
    s_base = atomicAdd(nlist, nfail);
  }
  if (!list || nfail == 0) return;   // uniform over the block
  __syncthreads();
  if (is[1]) {
    uint32_t pos = s_base + (uint32_t)__builtin_popcountll(mfail & ((1ull << lane) - 1ull));
    for (uint32_t w = 0; w < wv; ++w) pos += s_sum[w][1];
    list[pos] = (uint32_t)i;
  }
}

// ---------------------------------------------------------------------------------------
// Key generation and signing (crypto::generate_keypair / Signature::new, lib.rs:167-191;
// dalek Keypair::generate + ExpandedSecretKey::sign = RFC 8032)
// ---------------------------------------------------------------------------------------
// SHA-512 of nwords64 whole 64-bit words (<= 13, one block), words given big-endian.
__device__ __forceinline__ void sha512_words(uint64_t st[8], const uint64_t* m, int nwords64) {
  uint64_t w[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) w[i] = i < nwords64 ? m[i] : 0;
#pragma unroll
  for (int i = 0; i < 16; ++i)
    if (i == nwords64) w[i] = 0x8000000000000000ULL;
  w[15] = (uint64_t)nwords64 * 64;
  sha512_init(st);
  sha512_compress(st, w);
}

__device__ __forceinline__ uint64_t be64_of_le_words(const uint32_t* x, int i) {
  return ((uint64_t)bswap32(x[2 * i]) << 32) | bswap32(x[2 * i + 1]);
}

// Expanded secret: a = clamp(H(seed)[0..32]) mod l, prefix = H(seed)[32..64] (LE words).
__device__ __forceinline__ void expand_seed(sc& a, uint32_t prefix[8], const uint32_t seed[8]) {
  uint64_t m[4], st[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) m[i] = be64_of_le_words(seed, i);
  sha512_words(st, m, 4);
  uint32_t h[16];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    h[2 * i] = bswap32((uint32_t)(st[i] >> 32));
    h[2 * i + 1] = bswap32((uint32_t)st[i]);
  }
  h[0] &= 0xfffffff8u;
  h[7] = (h[7] & 0x7fffffffu) | 0x40000000u;
  uint32_t x[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) x[i] = i < 8 ? h[i] : 0u;
  sc_reduce512(a, x);   // [a]B = [a mod l]B
#pragma unroll
  for (int i = 0; i < 8; ++i) prefix[i] = h[8 + i];
}

__global__ __launch_bounds__(256) void k_keypair(const uint32_t* __restrict__ seeds, uint64_t n,
                                                 uint32_t* __restrict__ pks) {
  __shared__ ge_niels s_btab[129];
  load_btab(s_btab);
  __syncthreads();
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t seed[8], prefix[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) seed[j] = seeds[8 * i + j];
  sc a;
  expand_seed(a, prefix, seed);
  ge A;
  fixed_base_mul(A, a, s_btab);
  uint32_t Aw[8];
  ge_tobytes(Aw, A);
#pragma unroll
  for (int j = 0; j < 8; ++j) pks[8 * i + j] = Aw[j];
}

// sks: crypto::SecretKey bytes (seed || pk), stride sk_stride_words (16, or 0 = one key).
__global__ __launch_bounds__(256) void k_sign(const uint32_t* __restrict__ sks,
                                              uint32_t sk_stride_words,
                                              const uint32_t* __restrict__ msgs,
                                              uint32_t msg_stride_words, uint64_t n,
                                              uint32_t* __restrict__ sigs) {
  __shared__ ge_niels s_btab[129];
  load_btab(s_btab);
  __syncthreads();
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t seed[8], pk[8], M[8], prefix[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    seed[j] = sks[(uint64_t)sk_stride_words * i + j];
    pk[j] = sks[(uint64_t)sk_stride_words * i + 8 + j];
    M[j] = msgs[(uint64_t)msg_stride_words * i + j];
  }
  sc a;
  expand_seed(a, prefix, seed);
  // r = H(prefix || M) mod l
  uint64_t m[8], st[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    m[j] = be64_of_le_words(prefix, j);
    m[4 + j] = be64_of_le_words(M, j);
  }
  sha512_words(st, m, 8);
  uint32_t hx[16];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    hx[2 * j] = bswap32((uint32_t)(st[j] >> 32));
    hx[2 * j + 1] = bswap32((uint32_t)st[j]);
  }
  sc r;
  sc_reduce512(r, hx);
  ge R;
  fixed_base_mul(R, r, s_btab);
  uint32_t Rw[8];
  ge_tobytes(Rw, R);
  hram96(hx, Rw, pk, M);
  sc k, ka, s;
  sc_reduce512(k, hx);
  sc_mul(ka, k, a);
  sc_add(s, ka, r);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    sigs[16 * i + j] = Rw[j];
    sigs[16 * i + 8 + j] = s.w[j];
  }
}

// The same over messages of any length (RFC 8032 5.1.6, dalek's Keypair::sign(&[u8])): message i
// is lengths[i] bytes at data + offsets[i], any alignment. Both hashes are sha512_prefix_lane's
// (nw_sha512.hpp): r over prefix || M (8-word prefix), k over R || A || M (16 words), so M is read
// twice, the second time from cache. A is the key's second half as given, as in k_sign. One lane
// per item; a wave runs as long as its longest message.
__global__ __launch_bounds__(256) void k_sign_msgs(const uint32_t* __restrict__ sks,
                                                   uint32_t sk_stride_words,
                                                   const uint8_t* __restrict__ data,
                                                   const uint64_t* __restrict__ offsets,
                                                   const uint64_t* __restrict__ lengths,
                                                   uint64_t n, uint32_t* __restrict__ sigs) {
  __shared__ ge_niels s_btab[129];
  load_btab(s_btab);
  __syncthreads();
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t seed[8], pk[8], prefix[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    seed[j] = sks[(uint64_t)sk_stride_words * i + j];
    pk[j] = sks[(uint64_t)sk_stride_words * i + 8 + j];
  }
  const uint8_t* const msg = data + offsets[i];
  const uint64_t len = lengths[i];
  sc a;
  expand_seed(a, prefix, seed);
  uint32_t hx[16];
  sha512_prefix_lane<8>(hx, prefix, msg, len);
  sc r;
  sc_reduce512(r, hx);
  ge R;
  fixed_base_mul(R, r, s_btab);
  uint32_t Rw[8];
  ge_tobytes(Rw, R);
  sha512_hram_lane(hx, Rw, pk, msg, len);
  sc k, ka, s;
  sc_reduce512(k, hx);
  sc_mul(ka, k, a);
  sc_add(s, ka, r);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    sigs[16 * i + j] = Rw[j];
    sigs[16 * i + 8 + j] = s.w[j];
  }
}

}  // namespace nw

namespace nw {
// The strict kernel's wide B tables, built on the device once per process and device, in
// padded affine niels form, one lane per entry: fixed-base product over the 8-bit LDS table,
// then one inversion.
// out[h * n + j] = j * 2^(shift h) * B for h < ntab (shift 128: the ladder's two tables;
// shift 16: the keyed comb's sixteen).
__global__ __launch_bounds__(256) void k_btab_build(ge_niels_pad* __restrict__ out, uint32_t n,
                                                    uint32_t ntab, uint32_t shift) {
  __shared__ ge_niels s_btab[129];
  load_btab(s_btab);
  __syncthreads();
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (uint64_t)ntab * n) return;
  const uint32_t h = (uint32_t)(g / n), j = (uint32_t)(g % n);
  sc s;
#pragma unroll
  for (int i = 0; i < 8; ++i) s.w[i] = 0;
  const uint32_t bit = shift * h, wi = bit >> 5, sh = bit & 31;   // j < 2^24, bit <= 240
  s.w[wi] = j << sh;
  if (sh && wi < 7) s.w[wi + 1] = j >> (32 - sh);
  ge P;
  fixed_base_mul(P, s, s_btab);
  ge_niels nb;
  ge_to_niels(nb, P, g_consts.k.d2);
  out[g].n = nb;
  out[g].pad[0] = out[g].pad[1] = 0;
}
}  // namespace nw

// ---------------------------------------------------------------------------------------
// Host side: constants and launchers
// ---------------------------------------------------------------------------------------
namespace nw {

// The strict kernel's wide B tables (k_btab_build), one copy per device, indexed by HIP
// device id, built on the device the first time a strict launch needs them there (24-bit
// windows: 2 x 8,388,609 entries = 2.15 GB and ~0.2 s per device; lazily, so a process
// that initialises every device but verifies on one builds one table).
static constexpr int kMaxDevIds = 64;
static std::atomic<ge_niels_pad*> g_btw[kMaxDevIds];
static std::mutex g_btw_mu[kMaxDevIds];   // per device: devices build in parallel
static constexpr uint32_t kBtwPerHalf = bdigits<NW_BWIN>::ENTRIES;

static std::atomic<ge_niels_pad*> g_bcomb[kMaxDevIds];

hipError_t table_malloc(void** p, size_t bytes) {
  *p = nullptr;
  if (const char* e = getenv("NW_DEVICE_MEM_LIMIT")) {
    const unsigned long long lim = strtoull(e, nullptr, 10);
    if (lim && bytes > lim) return hipErrorOutOfMemory;
  }
  const hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess) {
    // reported by the return value; leave no last error behind for the next launch check
    *p = nullptr;
    (void)hipGetLastError();
  }
  return e;
}


// Table set `which` of the current device (0: the ladder's 2 x kBtwPerHalf; 1: the keyed
// comb's kBCombT x kBCombN: 11 x 8,388,609 = 11.8 GB at 24-bit digits), built on first use.
static hipError_t btab_for_current_device(int which, const ge_niels_pad** out) {
  *out = nullptr;
  if (which == 0 && NW_BWIN == 8) return hipSuccess;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev >= kMaxDevIds) return hipErrorInvalidDevice;
  std::atomic<ge_niels_pad*>& slot = which ? g_bcomb[dev] : g_btw[dev];
  if ((*out = slot.load(std::memory_order_acquire))) return hipSuccess;
  std::lock_guard<std::mutex> lock(g_btw_mu[dev]);
  if ((*out = slot.load(std::memory_order_relaxed))) return hipSuccess;
  const uint32_t n = which ? kBCombN : kBtwPerHalf, ntab = which ? kBCombT : 2;
  const uint32_t shift = which ? (uint32_t)kBCombW : 128;
  void* p = nullptr;
  const uint64_t entries = (uint64_t)ntab * n;
  e = table_malloc(&p, entries * sizeof(ge_niels_pad));
  if (e != hipSuccess) return e;
  hipStream_t s = nullptr;
  e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_btab_build, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, s,
                       static_cast<ge_niels_pad*>(p), n, ntab, shift);
    e = hipGetLastError();
    const hipError_t e2 = hipStreamSynchronize(s);
    if (e == hipSuccess) e = e2;
    (void)hipStreamDestroy(s);
  }
  if (e != hipSuccess) { (void)hipFree(p); return e; }
  slot.store(static_cast<ge_niels_pad*>(p), std::memory_order_release);
  *out = static_cast<ge_niels_pad*>(p);
  return hipSuccess;
}

hipError_t bcomb_table(const ge_niels_pad** out) { return btab_for_current_device(1, out); }

hipError_t prepare_strict_tables() {
  const ge_niels_pad* p = nullptr;
  hipError_t e = btab_for_current_device(0, &p);
  return e != hipSuccess ? e : btab_for_current_device(1, &p);
}

hipError_t upload_consts() {
  static dev_consts host;
  static std::once_flag once;
  std::call_once(once, [] {
    compute_consts(host.k, host.btab);
    compute_strict_consts(host.sk, host.b128);
  });
  hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(g_consts), &host, sizeof(host), 0,
                                   hipMemcpyHostToDevice);
  if (e == hipSuccess) e = upload_batch_consts();
  return e != hipSuccess ? e : upload_small_consts();
}

static inline unsigned grid_for(uint64_t n, unsigned block) {
  return (unsigned)((n + block - 1) / block);
}
// Chunks of a batched inversion over n items: ~2 waves per SIMD of lanes, each over
// n / chunks items (>= 1).
static inline uint64_t inv_chunks(uint64_t n) { return std::min<uint64_t>(n, 256ull * 4 * 2 * 64); }

hipError_t launch_sha512_digest32(const uint8_t* data, const uint64_t* offsets,
                                  const uint64_t* lengths, uint64_t n, uint32_t* out,
                                  hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_sha512_digest32, dim3(grid_for(n, 256)), dim3(256), 0, stream, data,
                     offsets, lengths, n, out);
  return hipGetLastError();
}

// Resident 256-thread blocks of k_verify_strict on the current device (occupancy query,
// once per device; concurrent first calls compute the same value).
static unsigned strict_grid() {
  static std::atomic<int> cached[64];
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev < 0 || dev >= 64) dev = 0;
  if (!cached[dev].load(std::memory_order_acquire)) {
    int per_cu = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_verify_strict<false>, 256, 0) !=
            hipSuccess || per_cu <= 0)
      per_cu = 1;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        cus <= 0)
      cus = 256;
    cached[dev].store(per_cu * cus, std::memory_order_release);
  }
  return (unsigned)cached[dev].load(std::memory_order_acquire);
}

// The keyed fast path reuses the per-lane table region for its limb planes (84 B per item of
// a slice) and keeps its list (4 B per item) and count in a tail after it.
constexpr uint64_t kKeyedSliceMax = 1ull << 22;
// (sized for 160-byte entries; the packed ones use 128 of each 160)
static size_t strict_tabs_bytes() { return (size_t)strict_grid() * 256 * 16 * sizeof(ge_cached); }
static bool env_is_zero(const char* name) {
  const char* e = getenv(name);
  return e && e[0] == '0';
}
bool strict_triage_on() {   // NW_STRICT_TRIAGE=0: one pass (k_verify_strict), A/B hook
  static const bool v = !env_is_zero("NW_STRICT_TRIAGE");
  return v;
}
static size_t strict_keyed_region_bytes() { return 4 * kKeyedSliceMax + 256; }
size_t strict_workspace_bytes() { return strict_tabs_bytes() + strict_keyed_region_bytes(); }
// The two-pass path's slice (k_strict_triage / k_verify_strict_pre): kTriagePlanes words and
// a list entry and a key slot per item, then the block and the key set
// (nw_strict_layout.hpp strict_region_plan); a region of its own, sized for the launch (176 B per item and 1 KB
// per key slot: 3.0 GB at the limit, 2.3 GB for config 4's 12.5M items). The limit is
// large: config 4 is one slice, so the second pass's last, partly filled round over the
// resident lanes comes once per launch.
constexpr uint64_t kTriageSlice = 1ull << 24;
static_assert(kTriageSlice <= (uint64_t)kTodoDecided,
              "a to-do entry holds the slice item below bit 31 (comb_todo_entry)");
uint64_t strict_triage_slice(uint64_t n, bool always) {
  if (!always && !strict_triage_on()) return 0;
  uint64_t lim = kTriageSlice;
  if (const char* e = getenv("NW_TRIAGE_SLICE")) {
    const unsigned long long v = strtoull(e, nullptr, 10);
    if (v >= 1 && v < lim) lim = v;
  }
  lim = (lim + 63) & ~63ull;
  return std::min<uint64_t>(lim, (std::max<uint64_t>(n, 1) + 63) & ~63ull);
}
// The slice's key set (nw_strict.hpp keyset_probe): slots of the open-addressing table, a power
// of two; at most half of them are filled. NW_STRICT_KEYS = slots (clamped to [64, 2^20] and
// rounded up to a power of two; 0 = no key set, the launch sequence without it), read per
// launch; default 2^16 (64 MB of tables), fewer for a small slice (strict_keys_plan).
uint64_t strict_keys_slots(uint64_t slice) {
  uint64_t req = kKeySlotsDefault;
  if (const char* e = getenv("NW_STRICT_KEYS")) req = strtoull(e, nullptr, 10);
  return strict_keys_plan(req, slice);
}
static_assert(kTriagePlanes == kTriagePlaneCount && sizeof(ge_cached_pk) * 8 == kKeyTabBytes,
              "strict_region_plan's layout");
size_t strict_triage_bytes(uint64_t slice, uint64_t key_slots) {
  return strict_region_plan(slice, key_slots).bytes;
}

// The comb path's region (nw_strict_layout.hpp) with the 8-bit tables of hot_cap keys.
static comb_region_t comb_plan(uint64_t slice, uint64_t key_slots, uint64_t hot_cap) {
  return comb_region_plan(slice, key_slots, hot_cap, key_tables_bytes(hot_cap, keyspec_for(8)));
}
size_t strict_comb_bytes(uint64_t slice, uint64_t key_slots, uint64_t hot_cap) {
  return comb_plan(slice, key_slots, hot_cap).bytes;
}

strict_launch_plan_t strict_launch_plan(uint64_t n, uint32_t registered, bool always) {
  strict_launch_plan_t p;
  if (n == 0 || (p.slice = strict_triage_slice(n, always)) == 0) return p;
  p.key_slots = strict_keys_slots(p.slice);
  // NW_STRICT_COMB_DECIDE=0: the comb path's to-do entries carry no verdict, so every listed
  // item that survives the triage takes the ladder (rounds 9-10's sequence; A/B hook)
  p.comb_decide = !env_is_zero("NW_STRICT_COMB_DECIDE");
  p.comb_min = 256;
  if (p.key_slots == 0 || env_is_zero("NW_STRICT_COMB")) return p;
  if (const char* e = getenv("NW_STRICT_COMB_MIN")) {
    const unsigned long long v = strtoull(e, nullptr, 10);
    p.comb_min = (uint32_t)std::min<unsigned long long>(std::max<unsigned long long>(v, 1), 1u << 30);
  }
  uint64_t keys = 8192;
  if (const char* e = getenv("NW_STRICT_COMB_KEYS")) keys = strtoull(e, nullptr, 10);
  p.hot_cap = std::min<uint64_t>({keys, p.slice / p.comb_min, 1ull << 20});
  p.signers = registered != 0 && n >= strict_signers_min_items();
  // key-major order of the comb path's lanes: small slices and slices of few keys have their
  // tables in the caches already and stay in item order
  if (p.comb()) {
    const char* e = getenv("NW_STRICT_KEY_MAJOR");
    const bool forced = e && e[0] != '\0' && e[0] != '0';
    p.key_major = forced || (!e && p.slice >= kKmAutoSlice);
    p.km_min_live = forced ? 1u : kKmAutoLive;
  }
  return p;
}
size_t strict_keymajor_bytes(uint64_t slice) { return km_region_plan(slice).bytes; }

// ---- diagnostics: the counters of the last unkeyed two-pass launch per device ----
namespace {
struct two_pass_record_t {
  const triage_block_t* triage = nullptr;   // counted only with a key set (keys_on)
  const comb_block_t* comb = nullptr;       // null: the comb path was off
  uint64_t n = 0;
  bool valid = false, keys_on = false;
  const km_block_t* km = nullptr;           // null: the launch ran in item order
};
std::mutex g_two_pass_m;
two_pass_record_t g_two_pass_last[64];
struct strict_counters_t {
  two_pass_record_t rec;   // !valid: no launch yet, nothing was read
  triage_block_t triage;   // read when rec.keys_on
  comb_block_t comb;       // read when rec.comb
  km_block_t km;           // read when rec.km
};
// Synchronises `stream`, then copies the blocks that the launch counted in.
hipError_t strict_last_counters(hipStream_t stream, strict_counters_t* s) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  {
    std::lock_guard<std::mutex> g(g_two_pass_m);
    s->rec = dev >= 0 && dev < 64 ? g_two_pass_last[dev] : two_pass_record_t{};
  }
  if (!s->rec.valid) return hipSuccess;
  e = hipStreamSynchronize(stream);
  if (e == hipSuccess && s->rec.keys_on)
    e = hipMemcpy(&s->triage, s->rec.triage, sizeof(s->triage), hipMemcpyDeviceToHost);
  if (e == hipSuccess && s->rec.comb)
    e = hipMemcpy(&s->comb, s->rec.comb, sizeof(s->comb), hipMemcpyDeviceToHost);
  if (e == hipSuccess && s->rec.km)
    e = hipMemcpy(&s->km, s->rec.km, sizeof(s->km), hipMemcpyDeviceToHost);
  return e;
}
template <size_t N>
uint64_t lane_sum(const unsigned long long (&lanes)[N]) {
  uint64_t t = 0;
  for (unsigned long long v : lanes) t += v;
  return t;
}
}  // namespace
hipError_t strict_keyset_stats(uint64_t out[3], hipStream_t stream) {
  strict_counters_t s;
  out[0] = out[1] = out[2] = 0;
  const hipError_t e = strict_last_counters(stream, &s);
  if (e != hipSuccess || !s.rec.valid) return e;
  if (s.rec.keys_on) {
    out[0] = s.triage.keys_tabulated;
    out[1] = lane_sum(s.triage.with_slot);
  }
  out[2] = s.rec.n - out[1];
  return hipSuccess;
}
hipError_t strict_comb_stats(uint64_t out[4], hipStream_t stream) {
  strict_counters_t s;
  out[0] = out[1] = out[2] = out[3] = 0;
  const hipError_t e = strict_last_counters(stream, &s);
  if (e != hipSuccess || !s.rec.valid) return e;
  out[3] = s.rec.n;
  if (!s.rec.comb) return hipSuccess;
  out[0] = s.comb.hot_keys;
  // k_strict_keyed<true>'s count, or k_strict_signers_count's lanes
  out[1] = s.comb.checked + lane_sum(s.comb.lane_checked);
  out[2] = s.rec.n - s.comb.listed;   // every item is either passed by the comb or listed
  out[3] = s.comb.listed;
  return hipSuccess;
}
hipError_t strict_decided_stats(uint64_t out[2], hipStream_t stream) {
  strict_counters_t s;
  out[0] = out[1] = 0;
  const hipError_t e = strict_last_counters(stream, &s);
  if (e != hipSuccess || !s.rec.valid || !s.rec.comb) return e;
  out[0] = lane_sum(s.comb.lane_settled);
  out[1] = s.comb.laddered;
  return hipSuccess;
}
hipError_t strict_keymajor_stats(uint64_t out[3], hipStream_t stream) {
  strict_counters_t s;
  out[0] = out[1] = out[2] = 0;
  const hipError_t e = strict_last_counters(stream, &s);
  if (e != hipSuccess || !s.rec.valid || !s.rec.km) return e;
  out[0] = s.km.placed;
  out[1] = s.km.bins;
  out[2] = s.km.slices;
  return hipSuccess;
}
hipError_t strict_signers_stats(uint64_t out[3], hipStream_t stream) {
  strict_counters_t s;
  out[0] = out[1] = out[2] = 0;
  const hipError_t e = strict_last_counters(stream, &s);
  if (e != hipSuccess || !s.rec.valid || !s.rec.comb) return e;
  out[0] = s.comb.matched;
  out[1] = lane_sum(s.comb.lane_reg_items);
  out[2] = lane_sum(s.comb.lane_reg_passed);
  return hipSuccess;
}

// ---- the registered signers (nw_kernels.h strict_signers_t) ----
uint64_t strict_signers_max() {
  if (const char* e = getenv("NW_STRICT_SIGNERS_MAX")) return strtoull(e, nullptr, 10);
  return 8192;
}
// Default 1: no measured size loses to the launch without the registry (DESIGN.md 5 "Round 10").
uint64_t strict_signers_min_items() {
  if (const char* e = getenv("NW_STRICT_SIGNERS_MIN_ITEMS")) return strtoull(e, nullptr, 10);
  return 1;
}
void strict_signers_free(strict_signers_t* sg) {
  if (sg->base) (void)hipFree(sg->base);
  *sg = strict_signers_t{};
}
hipError_t strict_signers_build(const uint8_t* keys32, uint32_t n, strict_signers_t* out,
                                hipStream_t stream) {
  *out = strict_signers_t{};
  if (n == 0) return hipSuccess;
  // host: the keys as words, the hash table, the identity rows and their count
  std::vector<uint32_t> keys(8 * (size_t)n), slots;
  memcpy(keys.data(), keys32, 32 * (size_t)n);
  const uint32_t cap = signers_hash_build(keys.data(), n, slots);
  if (cap == 0) return hipErrorInvalidValue;
  // one allocation: keys | slots | ok | rows | nlive | lam, then the tables (256-byte aligned)
  const keyspec ks8 = keyspec_for(8);
  const uint64_t o_slots = 32ull * n, o_ok = o_slots + 4ull * cap, o_rows = o_ok + 4ull * n,
                 o_live = o_rows + 4ull * n, o_lam = o_live + 4,
                 o_tabs = (o_lam + 4ull * n + 255) & ~255ull;
  void* base = nullptr;
  hipError_t e = table_malloc(&base, o_tabs + key_tables_bytes(n, ks8));
  if (e != hipSuccess) return e;
  char* const b = static_cast<char*>(base);
  std::vector<uint32_t> rows(n + 1);
  for (uint32_t r = 0; r < n; ++r) rows[r] = r;
  rows[n] = n;   // nlive, right behind the rows
  e = hipMemcpyAsync(b, keys.data(), 32 * (size_t)n, hipMemcpyHostToDevice, stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(b + o_slots, slots.data(), 4 * (size_t)cap, hipMemcpyHostToDevice, stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(b + o_rows, rows.data(), 4 * (size_t)(n + 1), hipMemcpyHostToDevice, stream);
  uint32_t* const ok = reinterpret_cast<uint32_t*>(b + o_ok);
  ge_niels_pad* const tabs = reinterpret_cast<ge_niels_pad*>(b + o_tabs);
  if (e == hipSuccess)
    e = launch_key_tables_rows(reinterpret_cast<const uint32_t*>(b),
                               reinterpret_cast<const uint32_t*>(b + o_rows),
                               reinterpret_cast<const uint32_t*>(b + o_live), n, ks8, tabs, ok,
                               stream);
  // each key's torsion image, for the plain batches (launch_batch_signers); `ok` keeps no lambda
  uint32_t* const lam = reinterpret_cast<uint32_t*>(b + o_lam);
  if (e == hipSuccess) e = launch_key_lambda(reinterpret_cast<const uint32_t*>(b), n, lam, stream);
  // the uploads read this function's vectors: they must have left before it returns
  const hipError_t e2 = hipStreamSynchronize(stream);
  if (e == hipSuccess) e = e2;
  if (e != hipSuccess) {
    (void)hipFree(base);
    return e;
  }
  out->base = base;
  out->keys = reinterpret_cast<const uint32_t*>(b);
  out->slots = reinterpret_cast<const uint32_t*>(b + o_slots);
  out->ok = ok;
  out->lam = lam;
  out->tabs = tabs;
  out->n = n;
  out->cap = cap;
  return hipSuccess;
}
// ---- launch_verify_strict: the two-pass launch, the one-pass launch, the keyed fast path ----
namespace {
struct strict_items_t {   // what a launch verifies, and where its verdicts go
  const uint32_t* msgs;
  uint32_t msg_stride_words;
  const uint32_t *pks, *sigs;
  uint64_t n;
  int32_t* status;
  uint64_t* bitmap;
  hipStream_t stream;
  // msgs is the k plane (launch_verify_strict_msgs: stride 8 words, k of item i at msgs + 8 i):
  // the two-pass launch runs its plane-reading instances of the kernels that evaluate k
  bool kplane = false;
};
// k_strict_todo_list and k_strict_signers_count: a block takes kTodoPer x 256 consecutive items
unsigned todo_grid(uint64_t ns) { return grid_for(ns, 256 * kTodoPer); }

// The launch's plan against what the allocations hold (Lease::strict_ws makes both).
bool strict_plan_fits(const strict_ws_t& ws, bool comb_on) {
  const strict_launch_plan_t& p = ws.plan;
  const strict_caps_t& c = ws.caps;
  if (!ws.triage || p.slice == 0 || c.slice < p.slice || p.key_slots > c.key_slots) return false;
  if (strict_triage_bytes(p.slice, p.key_slots) > strict_triage_bytes(c.slice, c.key_slots))
    return false;
  return !comb_on || (p.comb_min != 0 && strict_comb_bytes(p.slice, p.key_slots, p.hot_cap) <=
                                             strict_comb_bytes(c.slice, c.key_slots, c.hot_keys));
}

// One slice (items i0 .. i0 + ns) of the two-pass launch. cv is empty without the comb path.
hipError_t strict_two_pass_slice(const strict_items_t& in, const strict_ws_t& ws,
                                 const strict_region_view& tv, const comb_region_view& cv,
                                 const km_region_view& kv, const ge_niels_pad* btw,
                                 const ge_niels_pad* bcomb, uint64_t i0, uint64_t ns) {
  const strict_signers_t& sg = ws.signers;
  const uint64_t slice = ws.plan.slice;
  const uint32_t kcap = (uint32_t)ws.plan.key_slots, hot_cap = (uint32_t)ws.plan.hot_cap;
  hipStream_t const stream = in.stream;
  const dim3 lanes(256), per_item(grid_for(ns, 256)), per_slot(grid_for(kcap, 256));
  triage_block_t* const tb = tv.block;
  // the comb path's words that the triage and the ladder read and count in (null without it).
  // live: the word by which the slice's comb kernels, the to-do list and the triage see that the
  // slice has nothing for the comb: hot keys + registered keys with registered signers, hot
  // keys without them
  comb_block_t* const cb = cv.block;
  const bool reg_on = cb && sg.n != 0;
  uint32_t *todo_count = nullptr, *live = nullptr;
  unsigned long long *listed = nullptr, *settled = nullptr, *laddered = nullptr;
  if (cb) {
    todo_count = &cb->todo_count;
    live = reg_on ? &cb->nlive : &cb->nhot;
    listed = &cb->listed;
    settled = cb->lane_settled;
    laddered = &cb->laddered;
  }
  hipError_t e = hipMemsetAsync(tb, 0, kTriageSliceWordsBytes, stream);
  if (e != hipSuccess) return e;
  if (kcap) {
    // the slice's key set: each key's slot, then each slot's flags and table, once
    e = hipMemsetAsync(tv.slots, 0, 4 * (size_t)kcap, stream);
    if (e == hipSuccess && cb) e = hipMemsetAsync(cb, 0, kCombSliceWordsBytes, stream);
    if (e == hipSuccess && cb) e = hipMemsetAsync(cv.uses, 0, 4 * (size_t)kcap, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_strict_keys_probe, per_item, lanes, 0, stream, in.pks, i0, ns, tv.slots,
                       kcap, kcap / 2, &tb->nkeys, tv.keyslot, tb->with_slot, cv.uses);
    hipLaunchKernelGGL(k_strict_keys_build, per_slot, lanes, 0, stream, in.pks, i0, tv.slots, kcap,
                       tv.kflags, tv.ktabs, &tb->keys_tabulated);
  }
  if (cb) {
    // the slice's hot keys and their 8-bit comb tables, then the comb check of their items:
    // a pass is status 0 (k_strict_keyed, or k_strict_keyed_inv for the x parity); every
    // other item of the slice goes on the to-do list, with the comb's verdict in the entry
    // when its sum ran (the triage then settles the item without the ladder). X' / Z' and the
    // state use the region's planes 0-20, which the triage overwrites afterwards.
    if (reg_on)
      hipLaunchKernelGGL(k_strict_signers_match, per_slot, lanes, 0, stream, in.pks, i0, tv.slots,
                         kcap, tv.kflags, signers_view{sg.keys, sg.slots, sg.cap}, cv.match,
                         &cb->nlive, &cb->matched);
    hipLaunchKernelGGL(k_strict_comb_select, per_slot, lanes, 0, stream, tv.slots, kcap, tv.kflags,
                       cv.uses, ws.plan.comb_min, hot_cap, &cb->nhot, cv.hotidx, cv.hotrow,
                       &cb->hot_keys, reg_on ? cv.match : nullptr, reg_on ? sg.n : 0u,
                       reg_on ? &cb->nlive : nullptr);
    const keyspec ks8 = keyspec_for(8);
    e = launch_key_tables_rows(in.pks + 8 * i0, cv.hotrow, &cb->nhot, hot_cap, ks8, cv.tabs, cv.hok,
                               stream);
    if (e != hipSuccess) return e;
    // key-major order (kv is empty for a launch in item order): the comb kernels' lane p takes
    // item perm[p] and leaves X' / Z' and the state at position p; the kernels up to the to-do
    // list read them there. The sort and its readers decide alike, from *live, whether the
    // slice is sorted.
    const uint32_t km_min = ws.plan.km_min_live;
    if (kv.perm) {
      const km_keys_t kk{tv.keyslot, cv.hotidx, &cb->nhot, live, reg_on ? sg.n : 0u, hot_cap,
                         km_min};
      const dim3 per_chunk(grid_for(ns, kKmChunk));
      hipLaunchKernelGGL(k_km_hist, per_chunk, lanes, 0, stream, ns, kk, kv.hist);
      hipLaunchKernelGGL(k_km_scan, dim3(1), dim3(kKmBins), 0, stream, kv.hist, kv.cursor,
                         kv.block, live, km_min);
      hipLaunchKernelGGL(k_km_scatter, per_chunk, lanes, 0, stream, ns, kk, kv.cursor, kv.perm,
                         kv.pslot);
    }
    const vote_planes_t vp{tv.planes, tv.planes + 20 * slice, slice, kv.perm};
    const key_tables_t hk{cv.tabs, cv.hok, tv.keyslot, ks8};
    const km_order_t km{kv.pslot, tv.slots, km_min};
    if (reg_on)
      hipLaunchKernelGGL(in.kplane ? k_strict_keyed_signers_k : k_strict_keyed_signers, per_item,
                         lanes, 0, stream, in.msgs, in.msg_stride_words, in.pks, in.sigs, i0, ns,
                         in.status, hk, bcomb, vp, cv.hotidx, &cb->nhot, &cb->nlive, sg.tabs, sg.ok,
                         sg.n, km);
    else if (in.kplane)
      hipLaunchKernelGGL(k_strict_keyed_hot_k, per_item, lanes, 0, stream, in.msgs,
                         in.msg_stride_words, in.pks, in.sigs, i0, ns, in.status, hk, bcomb, vp, 0,
                         cv.hotidx, &cb->nhot, &cb->checked, km);
    else
      hipLaunchKernelGGL((k_strict_keyed<true, km_order_t>), per_item, lanes, 0, stream, in.msgs,
                         in.msg_stride_words, in.pks, in.sigs, i0, ns, in.status, hk, bcomb, vp, 0,
                         cv.hotidx, &cb->nhot, &cb->checked, km);
    const uint64_t nchunks = inv_chunks(ns);
    hipLaunchKernelGGL(k_strict_keyed_inv, dim3(grid_for(nchunks, 256)), lanes, 0, stream, i0, ns,
                       nchunks, in.status, vp, live, km_min);
    if (reg_on)
      hipLaunchKernelGGL(k_strict_signers_count, dim3(todo_grid(ns)), lanes, 0, stream, ns,
                         tv.keyslot, cv.hotidx, &cb->nhot, &cb->nlive, sg.n, vp.state,
                         cb->lane_checked, kv.perm, kv.pslot, km_min);
    hipLaunchKernelGGL(k_strict_todo_list, dim3(todo_grid(ns)), lanes, 0, stream, ns, vp.state,
                       cv.todo, todo_count, live, (uint32_t)ws.plan.comb_decide, kv.perm, km_min);
  }
  hipLaunchKernelGGL(in.kplane ? k_strict_triage_k : k_strict_triage, per_item, lanes, 0, stream,
                     in.msgs, in.msg_stride_words, in.pks, in.sigs, i0, ns, in.status, tv.planes,
                     slice, tv.list, &tb->count, tv.keyslot, tv.kflags, cv.todo, todo_count, listed,
                     live, settled);
  // (the ladder reads the scalar words the triage stored, never k: one instance serves both)
  hipLaunchKernelGGL(k_verify_strict_pre, dim3(std::min<uint64_t>(strict_grid(), per_item.x)),
                     lanes, 0, stream, in.msgs, in.msg_stride_words, in.pks, in.sigs, i0, tv.list,
                     &tb->count, tv.planes, slice, in.status, static_cast<ge_cached_pk*>(ws.base),
                     btw, tv.ktabs, laddered);
  return hipSuccess;
}

// The unkeyed launch in two passes (NW_STRICT_TRIAGE), slice by slice.
hipError_t launch_strict_two_pass(const strict_items_t& in, const strict_ws_t& ws,
                                  const ge_niels_pad* btw) {
  const strict_launch_plan_t& p = ws.plan;
  // the comb check needs its allocation (Lease::strict_ws plans none without one) and the B
  // comb; without either the launch runs without it
  const ge_niels_pad* bcomb = nullptr;
  const bool comb_on = ws.comb && p.comb() && p.key_slots &&
                       btab_for_current_device(1, &bcomb) == hipSuccess;
  if (!comb_on) bcomb = nullptr;
  if (!strict_plan_fits(ws, comb_on)) return hipErrorInvalidValue;
  const strict_region_view tv(ws.triage, strict_region_plan(p.slice, p.key_slots),
                              p.key_slots != 0);
  const comb_region_view cv =
      comb_on ? comb_region_view(ws.comb, comb_plan(p.slice, p.key_slots, p.hot_cap))
              : comb_region_view();
  // the launch's counters, kept over its slices
  hipError_t e = hipSuccess;
  if (p.key_slots)
    e = hipMemsetAsync(&tv.block->keys_tabulated, 0,
                       sizeof(triage_block_t) - kTriageSliceWordsBytes, in.stream);
  if (e == hipSuccess && cv.block)
    e = hipMemsetAsync(&cv.block->hot_keys, 0, sizeof(comb_block_t) - kCombSliceWordsBytes,
                       in.stream);
  // key-major order of the comb path's lanes: its region (Lease::strict_ws plans none without
  // one), the block, the histogram and the cursors cleared once per launch
  const km_region_view kv = comb_on && p.key_major && ws.keymajor && ws.caps.km_slice >= p.slice
                                ? km_region_view(ws.keymajor, km_region_plan(p.slice))
                                : km_region_view();
  if (e == hipSuccess && kv.block) e = hipMemsetAsync(kv.block, 0, kKmClearBytes, in.stream);
  if (e != hipSuccess) return e;
  int dev = 0;
  if (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64) {
    std::lock_guard<std::mutex> g(g_two_pass_m);
    g_two_pass_last[dev] =
        two_pass_record_t{tv.block, cv.block, in.n, true, p.key_slots != 0, kv.block};
  }
  // equal slices of at most p.slice items
  const uint64_t nsl = (in.n + p.slice - 1) / p.slice;
  const uint64_t per = (in.n + nsl - 1) / nsl;
  for (uint64_t i0 = 0; i0 < in.n; i0 += per) {
    e = strict_two_pass_slice(in, ws, tv, cv, kv, btw, bcomb, i0, std::min(per, in.n - i0));
    if (e != hipSuccess) return e;
  }
  if (in.bitmap)
    hipLaunchKernelGGL(k_status_bitmap, dim3(grid_for(in.n, 256)), dim3(256), 0, in.stream,
                       in.status, in.n, in.bitmap);
  return hipGetLastError();
}

// One pass of k_verify_strict over every item: the unkeyed launch with NW_STRICT_TRIAGE=0
// (bcomb null) and the committee-keyed one with NW_STRICT_KEYED_FAST=0.
hipError_t launch_strict_one_pass(const strict_items_t& in, void* workspace,
                                  const key_tables_t& kt, const ge_niels_pad* btw,
                                  const ge_niels_pad* bcomb) {
  const dim3 grid(std::min<uint64_t>(strict_grid(), grid_for(in.n, 256)));
  hipLaunchKernelGGL(kt.vote_key ? k_verify_strict<true> : k_verify_strict<false>, grid, dim3(256),
                     0, in.stream, in.msgs, in.msg_stride_words, in.pks, in.sigs, in.n, in.status,
                     in.bitmap, static_cast<ge_cached_pk*>(workspace), kt, btw, bcomb, nullptr,
                     nullptr);
  return hipGetLastError();
}

// The committee-keyed fast path (k_strict_keyed above), slice by slice through the workspace:
// the per-lane table region holds the slice's limb planes, the tail its list and count.
hipError_t launch_strict_keyed_fast(const strict_items_t& in, void* workspace,
                                    const key_tables_t& kt, const ge_niels_pad* btw,
                                    const ge_niels_pad* bcomb) {
  hipStream_t const stream = in.stream;
  const uint64_t S = std::min<uint64_t>(kKeyedSliceMax, strict_tabs_bytes() / (4 * 21)) & ~63ull;
  uint32_t* base = static_cast<uint32_t*>(workspace);
  uint32_t* list = reinterpret_cast<uint32_t*>(static_cast<char*>(workspace) + strict_tabs_bytes());
  uint32_t* count = list + kKeyedSliceMax;
  const vote_planes_t vp{base, base + 20 * S, S, nullptr};
  for (uint64_t i0 = 0; i0 < in.n; i0 += S) {
    const uint64_t ns = std::min(S, in.n - i0);
    const dim3 lanes(256), per_item(grid_for(ns, 256));
    hipError_t e = hipMemsetAsync(count, 0, 4, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_strict_keyed<false>, per_item, lanes, 0, stream, in.msgs,
                       in.msg_stride_words, in.pks, in.sigs, i0, ns, in.status, kt, bcomb, vp, i0,
                       nullptr, nullptr, nullptr);
    const uint64_t nchunks = inv_chunks(ns);
    hipLaunchKernelGGL(k_strict_keyed_inv, dim3(grid_for(nchunks, 256)), lanes, 0, stream, i0, ns,
                       nchunks, in.status, vp, nullptr, 0u);
    hipLaunchKernelGGL(k_strict_keyed_list, per_item, lanes, 0, stream, i0, ns, vp.state, list,
                       count);
    // the leftovers: full verification (exact status codes), the tables over the planes
    hipLaunchKernelGGL(k_verify_strict<true>, dim3(std::min<uint64_t>(strict_grid(), per_item.x)),
                       lanes, 0, stream, in.msgs, in.msg_stride_words, in.pks, in.sigs, ns,
                       in.status, in.bitmap, static_cast<ge_cached_pk*>(workspace), kt, btw, bcomb,
                       list, count);
  }
  if (in.bitmap)
    hipLaunchKernelGGL(k_status_bitmap, dim3(grid_for(in.n, 256)), dim3(256), 0, stream, in.status,
                       in.n, in.bitmap);
  return hipGetLastError();
}
}  // namespace

hipError_t launch_verify_strict(const uint32_t* msgs, uint32_t msg_stride_words,
                                const uint32_t* pks, const uint32_t* sigs, uint64_t n,
                                int32_t* status, uint64_t* bitmap, const strict_ws_t& ws,
                                hipStream_t stream, const key_tables_t* keys) {
  if (n == 0) return hipSuccess;
  const strict_items_t in{msgs, msg_stride_words, pks, sigs, n, status, bitmap, stream};
  const key_tables_t kt = keys ? *keys : key_tables_t{nullptr, nullptr, nullptr, {}};
  const ge_niels_pad* btw = nullptr;
  const ge_niels_pad* bcomb = nullptr;
  hipError_t e = btab_for_current_device(0, &btw);
  if (e == hipSuccess && kt.vote_key) e = btab_for_current_device(1, &bcomb);
  if (e != hipSuccess) return e;
  if (!kt.vote_key)
    return strict_triage_on() ? launch_strict_two_pass(in, ws, btw)
                              : launch_strict_one_pass(in, ws.base, kt, btw, nullptr);
  return env_is_zero("NW_STRICT_KEYED_FAST") ? launch_strict_one_pass(in, ws.base, kt, btw, bcomb)
                                             : launch_strict_keyed_fast(in, ws.base, kt, btw, bcomb);
}

hipError_t launch_strict_hram(const uint8_t* data, const uint64_t* offsets,
                              const uint64_t* lengths, const uint32_t* pks, const uint32_t* sigs,
                              uint64_t n, uint32_t* kplane, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (!kplane || !offsets || !lengths) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_strict_hram, dim3(grid_for(n, 256)), dim3(256), 0, stream, data, offsets,
                     lengths, pks, sigs, n, kplane);
  return hipGetLastError();
}

// The strict launch over messages of any length: k of every item into the plane, then the
// two-pass launch (always: NW_STRICT_TRIAGE=0 is an A/B hook of the 32-byte launch) with the
// plane in the place of the digests.
hipError_t launch_verify_strict_msgs(const uint8_t* data, const uint64_t* offsets,
                                     const uint64_t* lengths, const uint32_t* pks,
                                     const uint32_t* sigs, uint64_t n, int32_t* status,
                                     uint64_t* bitmap, const strict_ws_t& ws, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (!ws.kplane) return hipErrorInvalidValue;
  const ge_niels_pad* btw = nullptr;
  hipError_t e = btab_for_current_device(0, &btw);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_strict_hram, dim3(grid_for(n, 256)), dim3(256), 0, stream, data, offsets,
                     lengths, pks, sigs, n, ws.kplane);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  strict_items_t in{ws.kplane, 8, pks, sigs, n, status, bitmap, stream};
  in.kplane = true;
  return launch_strict_two_pass(in, ws, btw);
}

size_t votes_keyed_bytes_per_vote() { return 4 * 22; }   // 20 limb planes, state, perm
size_t votes_keyed_fixed_bytes() { return 4 * kVkMaxBins; }   // key histogram / cursors

hipError_t launch_votes_keyed(const uint32_t* cert_digest, const uint64_t* cvo, uint64_t ncert,
                              const uint32_t* vote_cert, const uint32_t* pks,
                              const uint32_t* sigs, uint64_t nvotes, const int32_t* pre1,
                              const int32_t* pre2, const int32_t* hdr_st,
                              const key_tables_t& keys, uint32_t nkeys, uint32_t* cert_ok,
                              void* scratch, size_t scratch_bytes, hipStream_t stream) {
  if (ncert == 0) return hipSuccess;
  if (!keys.vote_key || !keys.tabs || !keys.ok || !vote_cert) return hipErrorInvalidValue;
  const ge_niels_pad* bcomb = nullptr;
  hipError_t eb = btab_for_current_device(1, &bcomb);
  if (eb != hipSuccess) return eb;
  hipLaunchKernelGGL(k_votes_keyed_init, dim3(grid_for(ncert, 256)), dim3(256), 0, stream, cvo,
                     ncert, cert_ok);
  // slices of S votes through the scratch (the caller's verify_batch workspace, free until
  // the failed certificates' batches run)
  if (nvotes == 0) return hipGetLastError();   // e.g. genesis certificates: no votes
  if (scratch_bytes < votes_keyed_fixed_bytes()) return hipErrorInvalidValue;
  const uint64_t cap = (scratch_bytes - votes_keyed_fixed_bytes()) / votes_keyed_bytes_per_vote();
  const uint64_t S = nvotes <= cap ? nvotes : cap & ~63ull;
  if (nvotes && S == 0) return hipErrorInvalidValue;
  uint32_t* gh = static_cast<uint32_t*>(scratch);
  uint32_t* base = gh + kVkMaxBins;
  // key-major order for committees whose tables overflow the caches (>= 32 keys: 2.1 GB of
  // 16-bit tables; config 2 N = 100: 7.58 -> 9.11 M certs/s in round 3; N = 50 22.4 -> 23.3
  // in round 5, profiles/r05kw2, though round 3 measured it slower there) — below that the
  // cert-major order's coalesced signature reads win (round 3: N = 4 / 10: 143 / 74
  // unsorted vs 137 / 72 sorted). NW_VOTES_KEY_MAJOR=1 / 0 forces it on / off.
  const char* km = getenv("NW_VOTES_KEY_MAJOR");
  const bool sort = nkeys + 1 <= kVkMaxBins &&
                    (km ? km[0] == '1' : nkeys >= kVkSortMinKeys);
  uint32_t* perm = base + 21 * S;
  const vote_planes_t vp{base, base + 20 * S, S, sort ? perm : nullptr};
  for (uint64_t v0 = 0; v0 < nvotes; v0 += S) {
    const uint64_t nv = std::min(S, nvotes - v0);
    if (sort) {
      hipError_t e = hipMemsetAsync(gh, 0, 4 * (nkeys + 1), stream);
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL(k_vk_hist, dim3(grid_for(nv, kVkChunk)), dim3(256), 0, stream, vote_cert,
                         keys.vote_key, v0, nv, pre1, pre2, hdr_st, nkeys, gh);
      hipLaunchKernelGGL(k_vk_scan, dim3(1), dim3(64), 0, stream, gh, nkeys + 1);
      hipLaunchKernelGGL(k_vk_scatter, dim3(grid_for(nv, kVkChunk)), dim3(256), 0, stream, vote_cert,
                         keys.vote_key, v0, nv, pre1, pre2, hdr_st, nkeys, gh, perm);
    }
    hipLaunchKernelGGL(k_votes_keyed, dim3(grid_for(nv, 256)), dim3(256), 0, stream,
                       cert_digest, vote_cert, v0, nv, pks, sigs, pre1, pre2, hdr_st, keys, bcomb,
                       cert_ok, vp);
    // chunks: ~2 waves per SIMD of lanes, each over nv / nchunks votes (>= 1)
    const uint64_t nchunks = inv_chunks(nv);
    hipLaunchKernelGGL(k_votes_keyed_inv, dim3(grid_for(nchunks, 256)), dim3(256), 0, stream,
                       vote_cert, v0, nv, nchunks, cert_ok, vp);
  }
  return hipGetLastError();
}

// Scratch of launch_batch_signers: 20 limb planes and the state word per vote, a word per batch;
// then the list of the votes that did not pass, launch_verify_batch's list of live chunks
// (a word per vote each) and the two lists' counts.
size_t batch_signers_bytes(uint64_t nbatches, uint64_t nitems) {
  return 4 * (23 * nitems + nbatches + 2);
}
static_assert(kBatchSignersCounters == kBsCounters, "the counter block of a call");
bool batch_signers_votes() {
  const char* e = getenv("NW_BATCH_SIGNERS_VOTES");
  return !(e && e[0] == '0');
}
uint64_t batch_signers_min_votes() {
  if (const char* e = getenv("NW_BATCH_SIGNERS"))
    if (e[0] == '0') return ~0ull;
  if (const char* e = getenv("NW_BATCH_SIGNERS_MIN_VOTES")) return strtoull(e, nullptr, 10);
  return 1;
}
hipError_t launch_batch_signers(const uint32_t* digests, const uint64_t* offsets, uint64_t nbatches,
                                const uint32_t* pks, const uint32_t* sigs, uint64_t nitems,
                                const strict_signers_t& sg, const ge_niels_pad* bcomb,
                                void* scratch, unsigned long long* counters,
                                const uint32_t** batch_ok_out, hipStream_t stream,
                                batch_votes_t* votes_out, bool kplane) {
  if (nbatches == 0 || sg.n == 0 || !sg.lam || !bcomb) return hipErrorInvalidValue;
  if (nitems > 0xffffffffull) votes_out = nullptr;   // the list's entries are 32 bits
  uint32_t* const base = static_cast<uint32_t*>(scratch);
  const vote_planes_t vp{base, base + 20 * nitems, nitems, nullptr};
  uint32_t* const batch_ok = base + 21 * nitems;
  uint32_t* const list = batch_ok + nbatches;
  uint32_t* const nlist = list + 2 * nitems;
  hipLaunchKernelGGL(k_batch_signers_init, dim3(grid_for(nbatches, 256)), dim3(256), 0, stream,
                     nbatches, batch_ok, counters, votes_out ? nlist : nullptr);
  if (nitems) {
    if (kplane)
      hipLaunchKernelGGL(k_batch_signers_k, dim3(grid_for(nitems, 256)), dim3(256), 0, stream,
                         digests, offsets, nbatches, pks, sigs, nitems,
                         signers_view{sg.keys, sg.slots, sg.cap}, sg.ok, sg.lam, sg.tabs, bcomb,
                         batch_ok, vp);
    else
    hipLaunchKernelGGL(k_batch_signers, dim3(grid_for(nitems, 256)), dim3(256), 0, stream, digests,
                       offsets, nbatches, pks, sigs, nitems, signers_view{sg.keys, sg.slots, sg.cap},
                       sg.ok, sg.lam, sg.tabs, bcomb, batch_ok, vp);
    // chunks: ~2 waves per SIMD of lanes, each over nitems / nchunks votes (>= 1), the sizing of
    // the strict and certificate-vote launches. Below 131,072 votes that is a lane and an
    // inversion per pending vote: the lanes are idle otherwise, and chunks of 8 votes measured
    // slower where latency counts (a lone 10,000-vote call 0.311 against 0.294-0.306 ms, a 34-vote
    // call 0.257 against 0.240-0.242) and equal on 262,144 votes and above (profiles/r12a)
    const uint64_t nchunks = inv_chunks(nitems);
    hipLaunchKernelGGL(k_batch_signers_inv, dim3(grid_for(nchunks, 256)), dim3(256), 0, stream,
                       offsets, nbatches, nitems, nchunks, batch_ok, vp);
  }
  hipLaunchKernelGGL(k_batch_signers_count, dim3(grid_for(std::max(nitems, nbatches), 256)),
                     dim3(256), 0, stream, nitems, vp.state, nbatches, batch_ok, offsets, counters,
                     votes_out ? list : nullptr, nlist);
  if (votes_out) *votes_out = batch_votes_t{vp.state, list, nlist, list + nitems, nlist + 1};
  *batch_ok_out = batch_ok;
  return hipGetLastError();
}

hipError_t launch_cert_ok_headers(const int32_t* hdr_st, uint64_t ncert, uint32_t* cert_ok,
                                  hipStream_t stream) {
  if (ncert == 0) return hipSuccess;
  hipLaunchKernelGGL(k_cert_ok_headers, dim3(grid_for(ncert, 256)), dim3(256), 0, stream, hdr_st,
                     ncert, cert_ok);
  return hipGetLastError();
}

hipError_t launch_keypair(const uint32_t* seeds, uint64_t n, uint32_t* pks, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_keypair, dim3(grid_for(n, 256)), dim3(256), 0, stream, seeds, n, pks);
  return hipGetLastError();
}

hipError_t launch_sign(const uint32_t* sks, uint32_t sk_stride_words, const uint32_t* msgs,
                       uint32_t msg_stride_words, uint64_t n, uint32_t* sigs,
                       hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_sign, dim3(grid_for(n, 256)), dim3(256), 0, stream, sks, sk_stride_words,
                     msgs, msg_stride_words, n, sigs);
  return hipGetLastError();
}

hipError_t launch_sign_msgs(const uint32_t* sks, uint32_t sk_stride_words, const uint8_t* data,
                            const uint64_t* offsets, const uint64_t* lengths, uint64_t n,
                            uint32_t* sigs, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (!sks || !offsets || !lengths || !sigs) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_sign_msgs, dim3(grid_for(n, 256)), dim3(256), 0, stream, sks,
                     sk_stride_words, data, offsets, lengths, n, sigs);
  return hipGetLastError();
}

}  // namespace nw
