// hostcheck.hip — TEST INFRASTRUCTURE. Exposes the device arithmetic headers (compiled as
// host code) through a C ABI so tests/test_hostcheck.py can compare the exact field /
// point / scalar / ladder code the kernels run against the CPU oracle, without a GPU.
// SHA-512 is device-only, so the verification entry takes k = H(R||A||M) mod l as input.
#include <string.h>
#include <algorithm>
#include <vector>
#include "../narwhal_amd/csrc/nw_consts.hpp"
#include "../narwhal_amd/csrc/nw_ladder.hpp"
#include "../narwhal_amd/csrc/nw_strict_keymajor.hpp"
#include "limb_ops.hpp"
#include "sc_ops.hpp"

using namespace nw;

static curve_consts K;
static ge_niels BT[129];
static strict_consts SK;
static ge_niels B128[129];
static ge_niels_pad* BTW = nullptr;   // 16-bit-window tables (the kernel's default)
static const uint32_t BTW_N = (1u << 15) + 1;
static bool ready = false;
static void init() {
  if (!ready) {
    compute_consts(K, BT);
    compute_strict_consts(SK, B128);
    BTW = new ge_niels_pad[2 * BTW_N];
    compute_wide_btab(BTW, 16);
    ready = true;
  }
}

static void load8(uint32_t w[8], const uint8_t* b) { memcpy(w, b, 32); }
static void store8(uint8_t* b, const uint32_t w[8]) { memcpy(b, w, 32); }

extern "C" {

int hc_decompress(const uint8_t in[32], uint8_t out[32]) {
  init();
  uint32_t w[8]; load8(w, in);
  ge p;
  if (!ge_frombytes(p, w, K)) return 0;
  uint32_t o[8]; ge_tobytes(o, p); store8(out, o);
  return 1;
}

int hc_is_small_order(const uint8_t in[32]) {
  init();
  uint32_t w[8]; load8(w, in);
  ge p;
  if (!ge_frombytes(p, w, K)) return -1;
  return ge_is_small_order(p) ? 1 : 0;
}

void hc_reduce512(const uint8_t in[64], uint8_t out[32]) {
  uint32_t x[16]; memcpy(x, in, 64);
  sc r; sc_reduce512(r, x); store8(out, r.w);
}

void hc_scalar_mul(const uint8_t a[32], const uint8_t b[32], uint8_t out[32]) {
  sc x, y, r; load8(x.w, a); load8(y.w, b); sc_mul(r, x, y); store8(out, r.w);
}

void hc_scalar_add(const uint8_t a[32], const uint8_t b[32], uint8_t out[32]) {
  sc x, y, r; load8(x.w, a); load8(y.w, b); sc_add(r, x, y); store8(out, r.w);
}

int hc_scalar_canonical(const uint8_t a[32]) { sc x; load8(x.w, a); return sc_is_canonical(x); }

void hc_fixed_base(const uint8_t s[32], uint8_t out[32]) {
  init();
  sc x; load8(x.w, s);
  ge r; fixed_base_mul(r, x, BT);
  uint32_t o[8]; ge_tobytes(o, r); store8(out, o);
}

// [b]B + [a]P
int hc_dsm(const uint8_t a[32], const uint8_t P[32], const uint8_t b[32], uint8_t out[32]) {
  init();
  uint32_t w[8]; load8(w, P);
  ge p;
  if (!ge_frombytes(p, w, K)) return 0;
  ge_cached tab[9]; build_table9(tab, p, K.d2);
  sc x, y; load8(x.w, a); load8(y.w, b);
  ge r; dsm_var_base(r, tab, x, y, BT);
  uint32_t o[8]; ge_tobytes(o, r); store8(out, o);
  return 1;
}

// Strict verification with the kernel's check order; k supplied (device-only SHA).
int hc_verify_strict(const uint8_t pk[32], const uint8_t sig[64], const uint8_t k32[32]) {
  init();
  uint32_t Aw[8], Rw[8], Sw[8];
  load8(Aw, pk); load8(Rw, sig); load8(Sw, sig + 32);
  const bool s_high = (Sw[7] >> 29) != 0;
  sc s; memcpy(s.w, Sw, 32);
  const bool s_canon = sc_is_canonical(s);
  ge A, R;
  const bool okA = ge_frombytes(A, Aw, K);
  const bool okR = ge_frombytes(R, Rw, K);
  const bool smallA = ge_is_small_order(A), smallR = ge_is_small_order(R);
  sc k; load8(k.w, k32);
  ge mA; ge_neg(mA, A);
  ge_cached tab[9]; build_table9(tab, mA, K.d2);
  if (!s_canon || s_high) memset(s.w, 0, 32);
  ge acc; dsm_var_base(acc, tab, k, s, BT);
  const bool eq = ge_eq_affine(acc, R);
  if (s_high) return 1;
  if (!okA) return 3;
  if (!s_canon) return 2;
  if (!okR) return 4;
  if (smallR) return 6;
  if (smallA) return 5;
  if (!eq) return 7;
  return 0;
}


// Half-size scalar split (nw_scalar.hpp): u (32 bytes), |v| (20 bytes), sign.
int hc_half_split(const uint8_t k32[32], uint8_t u32[32], uint8_t v20[20]) {
  sc k; load8(k.w, k32);
  sc_half h; sc_half_split(h, k);
  memcpy(u32, h.u, 32); memcpy(v20, h.v, 20);
  return h.vneg ? 1 : 0;
}

// The same split by single Euclid steps only (the reference for the Lehmer rounds).
int hc_half_split_onestep(const uint8_t k32[32], uint8_t u32[32], uint8_t v20[20]) {
  sc k; load8(k.w, k32);
  sc_half h; sc_half_split<false>(h, k);
  memcpy(u32, h.u, 32); memcpy(v20, h.v, 20);
  return h.vneg ? 1 : 0;
}

// The kernel's strict verification (nw_strict.hpp), k supplied (device-only SHA), with
// B windows of bw = 16 bits (wide tables; the host-built copy), 8 bits (LDS tables) or
// 20 / 24 bits (entries computed per lookup). bw < 0: |bw| with the per-lane tables packed
// into 128-byte entries (ge_cached_pk, NW_PACK_TAB).
int hc_verify_strict_half(const uint8_t pk[32], const uint8_t sig[64], const uint8_t k32[32],
                          int bw) {
  init();
  uint32_t Aw[8], Rw[8], Sw[8];
  load8(Aw, pk); load8(Rw, sig); load8(Sw, sig + 32);
  uint32_t kw[8]; load8(kw, k32);
  ge_cached ta[8], tr[8];
  const strict_src_arrays src{Aw, Rw, Sw, kw};
  auto id = [](int w) { return w; };
  if (bw < 0) {
    ge_cached_pk pa[8], pr[8];
    if (bw == -24) return strict_verify_core<24>(src, SK, btab_lazy{BT, &SK.k.d2}, pa, pr, id);
    return strict_verify_core<16>(src, SK, btab_wide{BTW, BTW_N}, pa, pr, id);
  }
  if (bw == 8) return strict_verify_core<8>(src, SK, btab_pair{BT, B128}, ta, tr, id);
  if (bw == 20) return strict_verify_core<20>(src, SK, btab_lazy{BT, &SK.k.d2}, ta, tr, id);
  if (bw == 24) return strict_verify_core<24>(src, SK, btab_lazy{BT, &SK.k.d2}, ta, tr, id);
  return strict_verify_core<16>(src, SK, btab_wide{BTW, BTW_N}, ta, tr, id);
}

// Config 4 in two passes, on the host: strict_triage (k_strict_triage's checks), then, for an
// item that passes them, strict_verify_core on the stored x of A and R (the kPre source, as
// k_verify_strict_pre's strict_src_pre) with B windows of |bw| bits and packed tables as
// hc_verify_strict_half(bw < 0). Must equal the one-pass status for every input.
struct src_arrays_pre : strict_src_arrays {
  static constexpr bool kPre = true;
  fe xa, xr;
  bool point(int pt, ge& P) const {
    uint32_t w[8];
    if (pt) R(w); else A(w);
    fe_frombytes(P.Y, w);
    P.X = pt ? xr : xa;
    fe_1(P.Z);
    fe_mul(P.T, P.X, P.Y);
    return true;
  }
};
int hc_verify_strict_twopass(const uint8_t pk[32], const uint8_t sig[64], const uint8_t k32[32],
                             int bw) {
  init();
  uint32_t Aw[8], Rw[8], Sw[8], kw[8];
  load8(Aw, pk); load8(Rw, sig); load8(Sw, sig + 32); load8(kw, k32);
  src_arrays_pre src{};
  src.a = Aw; src.r = Rw; src.s = Sw; src.k = kw;
  const int st = strict_triage(static_cast<const strict_src_arrays&>(src), SK, src.xa, src.xr);
  if (st != NW_OK) return st;
  ge_cached_pk pa[8], pr[8];
  auto id = [](int w) { return w; };
  if (bw == -24) return strict_verify_core<24>(src, SK, btab_lazy{BT, &SK.k.d2}, pa, pr, id);
  return strict_verify_core<16>(src, SK, btab_wide{BTW, BTW_N}, pa, pr, id);
}

// Host model of the ladder's LDS prefetcher (nw_kernels.hip pf_lds; nw_strict.hpp pf_none for
// the contract), so the branch of strict_verify_core the device runs (PF::enabled, digit
// words through dput / dget, every entry requested one addition ahead) runs on the CPU too.
// One 128-byte slot: issue() copies the entry in, get() / get_signed() read it and then
// poison it, so a read without a matching request, or a second read of the same request,
// yields garbage limbs instead of the right entry. The digit words are an array, garbage
// until put.
struct pf_host_state {
  uint32_t slot[32];
  uint32_t dig[kStrictDigitWords];
  uint32_t poison_seq = 0x9e3779b9u;
  pf_host_state() {
    poison();
    for (int t = 0; t < kStrictDigitWords; ++t) dig[t] = 0x5a5a5a5au + 0x01010101u * (uint32_t)t;
  }
  void poison() {
    for (int i = 0; i < 32; ++i) slot[i] = (poison_seq = poison_seq * 1664525u + 1013904223u);
  }
};
struct pf_host {
  static constexpr bool enabled = true;
  static constexpr bool lds_digits = true;
  pf_host_state* st;
  void dput(int k, uint32_t v) const { st->dig[k] = v; }
  uint32_t dget(int k) const { return st->dig[k]; }
  void issue(const void* src, int chunks) const {
    memcpy(st->slot, src, 16 * (size_t)(chunks < 8 ? chunks : 8));
  }
  void read(ge_cached& e, bool niels, uint32_t a) const {
    uint32_t p[32];
    for (int k = 0; k < 8; ++k) memcpy(p + 4 * k, st->slot + 4 * (k < 4 ? (k ^ a) : k), 16);
    st->poison();
    if (niels) {
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
  void get(ge_cached& e, bool niels) const { read(e, niels, 0u); }
  void get_signed(ge_cached& e, bool neg) const { read(e, false, neg ? 2u : 0u); }
};
// btab_lazy with the entry() the prefetch branch asks for: the entry computed into a buffer
// of the table's own (issue() copies it at once).
struct btab_lazy_entry {
  btab_lazy lazy;
  mutable ge_niels_pad buf;
  const ge_niels_pad* entry(int h, int ad) const {
    ge_cached e;
    lazy(h, ad, e);
    memset(&buf, 0, sizeof(buf));
    fe_copy(buf.n.ypx, e.YpX);
    fe_copy(buf.n.ymx, e.YmX);
    fe_copy(buf.n.xy2d, e.T2d);
    return &buf;
  }
  void operator()(int h, int ad, ge_cached& e) const { lazy(h, ad, e); }
};

// hc_verify_strict_half(bw < 0) through the prefetch branch (bw = -16 or -24).
int hc_verify_strict_half_pf(const uint8_t pk[32], const uint8_t sig[64], const uint8_t k32[32],
                             int bw) {
  init();
  uint32_t Aw[8], Rw[8], Sw[8], kw[8];
  load8(Aw, pk); load8(Rw, sig); load8(Sw, sig + 32); load8(kw, k32);
  const strict_src_arrays src{Aw, Rw, Sw, kw};
  auto id = [](int w) { return w; };
  ge_cached_pk pa[8], pr[8];
  pf_host_state st;
  if (bw == -24)
    return strict_verify_core<24>(src, SK, btab_lazy_entry{{BT, &SK.k.d2}, {}}, pa, pr, id,
                                  pf_host{&st});
  return strict_verify_core<16>(src, SK, btab_wide{BTW, BTW_N}, pa, pr, id, pf_host{&st});
}

// Config 4 in two passes as the device runs them: strict_triage, then for a survivor the
// triage-side scalar phase (strict_triage_scalars: the 21 digit words, vneg and W stored),
// then the ladder from the stored x and the stored words (kPre and kScalars, as
// strict_src_pre) through the prefetch branch.
struct src_arrays_pre_scalars : src_arrays_pre {
  static constexpr bool kScalars = true;
  uint32_t words[kStrictDigitWords + 1];
  uint32_t digit_word(int t) const { return words[t]; }
  uint32_t scalar_meta() const { return words[kStrictDigitWords]; }
};
extern "C++" {
template <int BW, class BTab>
static int twopass_scalars(src_arrays_pre_scalars& src, const BTab& bt) {
  const int st = strict_triage(static_cast<const strict_src_arrays&>(src), SK, src.xa, src.xr);
  if (st != NW_OK) return st;
  strict_triage_scalars<BW>(static_cast<const strict_src_arrays&>(src), src.words,
                            src.words[kStrictDigitWords]);
  ge_cached_pk pa[8], pr[8];
  pf_host_state ps;
  return strict_verify_core<BW>(src, SK, bt, pa, pr, [](int w) { return w; }, pf_host{&ps});
}
}
int hc_verify_strict_twopass_scalars(const uint8_t pk[32], const uint8_t sig[64],
                                     const uint8_t k32[32], int bw) {
  init();
  uint32_t Aw[8], Rw[8], Sw[8], kw[8];
  load8(Aw, pk); load8(Rw, sig); load8(Sw, sig + 32); load8(kw, k32);
  src_arrays_pre_scalars src{};
  src.a = Aw; src.r = Rw; src.s = Sw; src.k = kw;
  if (bw == -24) return twopass_scalars<24>(src, btab_lazy_entry{{BT, &SK.k.d2}, {}});
  return twopass_scalars<16>(src, btab_wide{BTW, BTW_N});
}

// The keyed strict path (nw_strict.hpp strict_keyed_comb): the key's comb table entries
// j * 2^(W t) A computed per lookup (keytab_lazy) by the definition the device's k_key_base /
// k_key_tabs tabulate, the B comb likewise. Returns the status; -1 when A does not decode is reported through the
// key flags exactly as the device does (status 3).
static const torsion_consts& torsion() {
  static torsion_consts tc;
  static bool have = false;
  if (!have) { compute_torsion(tc); have = true; }
  return tc;
}
static uint32_t keyed_key(ge& A, const uint32_t Aw[8]) {
  const bool dec = ge_frombytes(A, Aw, K);
  // [l] A == [lambda] T8, the text k_key_base and k_key_lambda run (nw_strict.hpp key_lambda)
  const uint32_t lam = dec ? key_lambda(A, L_W, K.d2, torsion()) : 0u;
  return (dec ? kKeyDecoded : 0u) | (dec && ge_is_small_order(A) ? kKeySmall : 0u) |
         (lam << kKeyLambdaShift);
}

// lambda of a key (bits 2..4 of the flag word): [l] A == [lambda] T8; -1 if A does not decode.
int hc_key_lambda(const uint8_t pk[32]) {
  init();
  uint32_t Aw[8];
  load8(Aw, pk);
  ge A;
  const uint32_t f = keyed_key(A, Aw);
  return (f & kKeyDecoded) ? (int)((f & kKeyLambdaMask) >> kKeyLambdaShift) : -1;
}

// Comb width of the keyed checks' (lazily computed) key tables: 16, 20 or 24 (the widths the
// device builds for a committee, nw_api.cpp key_width) or 8 (a strict launch's hot keys).
static uint32_t g_key_w = 16;
int hc_set_key_width(int w) {
  if (w != 8 && w != 16 && w != 20 && w != 24) return -1;
  g_key_w = (uint32_t)w;
  return 0;
}

int hc_verify_strict_keyed(const uint8_t pk[32], const uint8_t sig[64], const uint8_t k32[32]) {
  init();
  uint32_t Aw[8], Rw[8], Sw[8], kw[8];
  load8(Aw, pk); load8(Rw, sig); load8(Sw, sig + 32); load8(kw, k32);
  ge A;
  const uint32_t flags = keyed_key(A, Aw);
  const strict_src_arrays src{Aw, Rw, Sw, kw};
  return strict_keyed_comb(src, SK, bcomb_lazy{BT, &SK.k.d2}, keytab_lazy{&A, &SK.k.d2, keyspec_for(g_key_w)}, flags);
}

// The certificate-vote keyed check without R decompression (nw_strict.hpp
// keyed_vote_check) followed by what k_votes_keyed_inv does for a pending vote (here one
// inversion per vote): 0 = the vote passes, 1 = it fails.
int hc_keyed_vote_check(const uint8_t pk[32], const uint8_t sig[64], const uint8_t k32[32]) {
  init();
  uint32_t Aw[8], Rw[8], Sw[8], kw[8];
  load8(Aw, pk); load8(Rw, sig); load8(Sw, sig + 32); load8(kw, k32);
  ge A;
  const uint32_t flags = keyed_key(A, Aw);
  const strict_src_arrays src{Aw, Rw, Sw, kw};
  fe X, Z;
  const uint32_t st = keyed_vote_check(src, SK, bcomb_lazy{BT, &SK.k.d2},
                                       keytab_lazy{&A, &SK.k.d2, keyspec_for(g_key_w)}, flags, X, Z);
  if (st < kVotePending) return (int)st;
  fe zi, x;
  fe_invert(zi, Z);
  fe_mul(x, X, zi);
  return fe_isnegative(x) == (st & 1) ? 0 : 1;
}

// Config 4's two passes with the call's key set, as launch_verify_strict runs a slice:
// keyset_probe for every item (the "atomics" are plain loads and stores: one thread), then
// keyset_build for every slot, then per item strict_triage on the slot's flags,
// strict_triage_scalars, and the ladder with the slot's table for tabA (the prefetch branch;
// a slotted item's per-lane table is left as garbage). The key set lies in one allocation at
// the offsets of strict_region_plan, sized as Lease::strict_ws sizes it. key_slots: as
// NW_STRICT_KEYS (0 = off); bw = -16 or -24. keyslot_out (n words, optional): each item's
// slot or kNoSlot; stats: keys tabulated, items with a slot, items without.
struct plain_atomics {
  uint32_t load(const uint32_t* p) const { return *p; }
  uint32_t cas(uint32_t* p, uint32_t expect, uint32_t val) const {
    const uint32_t old = *p;
    if (old == expect) *p = val;
    return old;
  }
  void inc(uint32_t* p) const { ++*p; }
};
struct src_arrays_keys : src_arrays_pre_scalars {
  static constexpr bool kSharedA = true;
  const ge_cached_pk* ktabs;
  uint32_t shared_slot() const {
    return (words[kStrictDigitWords] & kMetaSharedA) ? xa.v[0] : kNoSlot;
  }
  const void* shared_tabs() const { return ktabs; }
  uint32_t scalar_meta() const { return words[kStrictDigitWords] & ~kMetaSharedA; }
};
extern "C++" {
template <int BW, class BTab>
static int keyset_item(src_arrays_keys& src, const BTab& bt, uint32_t slot, const uint32_t* kflags,
                       bool* laddered = nullptr) {
  const uint32_t keyflags = slot != kNoSlot ? kflags[slot] : kNoSlot;
  for (int t = 0; t < 10; ++t) src.xa.v[t] = 0xdeadbeefu;
  const int st = strict_triage(static_cast<const strict_src_arrays&>(src), SK, src.xa, src.xr,
                               keyflags, [](bool b) { return b; });
  if (laddered) *laddered = st == NW_OK;
  if (st != NW_OK) return st;
  if (slot != kNoSlot) src.xa.v[0] = slot;
  strict_triage_scalars<BW>(static_cast<const strict_src_arrays&>(src), src.words,
                            src.words[kStrictDigitWords]);
  if (slot != kNoSlot) src.words[kStrictDigitWords] |= kMetaSharedA;
  ge_cached_pk pa[8], pr[8];
  memset(pa, 0xa5, sizeof(pa));
  pf_host_state ps;
  return strict_verify_core<BW>(src, SK, bt, pa, pr, [](int w) { return w; }, pf_host{&ps});
}
}
int hc_verify_strict_keyset_many(const uint8_t* pks, const uint8_t* sigs, const uint8_t* k32,
                                 uint32_t n, uint64_t key_slots, int bw, int32_t* status_out,
                                 uint32_t* keyslot_out, uint64_t stats[3]) {
  init();
  if (n == 0) return 0;
  const uint64_t slice = ((uint64_t)n + 63) & ~63ull;
  const uint32_t cap = (uint32_t)strict_keys_plan(key_slots, slice);
  const strict_region_t rg = strict_region_plan(slice, cap);
  // only the parts this check uses are touched; the planes before them stay unallocated
  const uint64_t first = rg.keyslot;
  uint8_t* mem = static_cast<uint8_t*>(malloc(rg.bytes - first));
  if (!mem) return -1;
  uint32_t* keyslot = reinterpret_cast<uint32_t*>(mem + (rg.keyslot - first));
  uint32_t* nkeys = reinterpret_cast<uint32_t*>(mem + (rg.block - first)) + 1;
  uint32_t* slots = reinterpret_cast<uint32_t*>(mem + (rg.slots - first));
  uint32_t* kflags = reinterpret_cast<uint32_t*>(mem + (rg.kflags - first));
  ge_cached_pk* ktabs = reinterpret_cast<ge_cached_pk*>(mem + (rg.ktabs - first));
  // the keys as aligned words (the device's pks array)
  uint32_t* pkw = static_cast<uint32_t*>(malloc(32 * (size_t)n));
  if (!pkw) { free(mem); return -1; }
  memcpy(pkw, pks, 32 * (size_t)n);
  *nkeys = 0;
  memset(slots, 0, 4 * (size_t)cap);
  uint64_t with = 0, owned = 0;
  for (uint32_t j = 0; j < n; ++j) {
    keyslot[j] = cap ? keyset_probe(slots, cap, cap / 2, nkeys, pkw, 0, j, plain_atomics{})
                     : kNoSlot;
    with += keyslot[j] != kNoSlot;
  }
  for (uint32_t s = 0; s < cap; ++s) {
    owned += slots[s] != 0;
    keyset_build(slots, s, pkw, 0, SK, kflags, ktabs);
  }
  for (uint32_t j = 0; j < n; ++j) {
    uint32_t Aw[8], Rw[8], Sw[8], kw[8];
    load8(Aw, pks + 32 * (size_t)j); load8(Rw, sigs + 64 * (size_t)j);
    load8(Sw, sigs + 64 * (size_t)j + 32); load8(kw, k32 + 32 * (size_t)j);
    src_arrays_keys src{};
    src.a = Aw; src.r = Rw; src.s = Sw; src.k = kw;
    src.ktabs = ktabs;
    status_out[j] = bw == -24
        ? keyset_item<24>(src, btab_lazy_entry{{BT, &SK.k.d2}, {}}, keyslot[j], kflags)
        : keyset_item<16>(src, btab_wide{BTW, BTW_N}, keyslot[j], kflags);
    if (keyslot_out) keyslot_out[j] = keyslot[j];
  }
  if (stats) { stats[0] = owned; stats[1] = with; stats[2] = n - with; }
  free(pkw);
  free(mem);
  return 0;
}
// A slice the way launch_verify_strict runs it with the comb check of the hot keys: the key
// set's probe with the sampled use counts, the slots' flags and tables, the hot keys in slot
// order up to comb_keys (the device hands out its indices by atomic ticket), keyed_vote_check
// with the hot key's 8-bit comb (keytab_lazy, no lambda: the flags are kKeyDecoded alone) and
// the parity by one inversion per item, then everything that did not pass through
// keyset_item. comb_min = 0 turns the path off. stats: hot keys, items checked, items passed,
// items sent on.
int hc_verify_strict_comb_many(const uint8_t* pks, const uint8_t* sigs, const uint8_t* k32,
                               uint32_t n, uint64_t key_slots, int bw, uint32_t comb_min,
                               uint32_t comb_keys, int32_t* status_out, uint64_t stats[4]) {
  init();
  if (n == 0) return 0;
  const uint64_t slice = ((uint64_t)n + 63) & ~63ull;
  const uint32_t cap = (uint32_t)strict_keys_plan(key_slots, slice);
  std::vector<uint32_t> keyslot(n), slots(cap), kflags(cap), uses(cap), hotidx(cap, kNoKey);
  std::vector<ge_cached_pk> ktabs(8 * (size_t)cap);
  std::vector<uint32_t> pkw(8 * (size_t)n);
  memcpy(pkw.data(), pks, 32 * (size_t)n);
  uint32_t nkeys = 0;
  for (uint32_t j = 0; j < n; ++j) {
    keyslot[j] = cap ? keyset_probe(slots.data(), cap, cap / 2, &nkeys, pkw.data(), 0, j,
                                    plain_atomics{})
                     : kNoSlot;
    if (keyslot[j] != kNoSlot && comb_sampled(j)) uses[keyslot[j]] += kCombSample;
  }
  for (uint32_t s = 0; s < cap; ++s)
    keyset_build(slots.data(), s, pkw.data(), 0, SK, kflags.data(), ktabs.data());
  const uint64_t hot_cap = comb_min ? std::min<uint64_t>(comb_keys, slice / comb_min) : 0;
  std::vector<ge> hotA;
  for (uint32_t s = 0; s < cap && hotA.size() < hot_cap; ++s) {
    if (slots[s] == 0 || !comb_key_hot(uses[s], comb_min, kflags[s])) continue;
    ge A;
    if (!ge_frombytes(A, pkw.data() + 8 * (size_t)(slots[s] - 1), K)) return -2;
    hotidx[s] = (uint32_t)hotA.size();
    hotA.push_back(A);
  }
  uint64_t checked = 0, passed = 0;
  const keyspec ks8 = keyspec_for(8);
  for (uint32_t j = 0; j < n; ++j) {
    uint32_t Aw[8], Rw[8], Sw[8], kw[8];
    load8(Aw, pks + 32 * (size_t)j); load8(Rw, sigs + 64 * (size_t)j);
    load8(Sw, sigs + 64 * (size_t)j + 32); load8(kw, k32 + 32 * (size_t)j);
    const uint32_t h = keyslot[j] != kNoSlot ? hotidx[keyslot[j]] : kNoKey;
    if (h != kNoKey) {
      ++checked;
      const strict_src_arrays src{Aw, Rw, Sw, kw};
      fe X, Z;
      uint32_t st = keyed_vote_check(src, SK, bcomb_lazy{BT, &SK.k.d2},
                                     keytab_lazy{&hotA[h], &SK.k.d2, ks8}, kKeyDecoded, X, Z);
      if (st >= kVotePending) {
        fe zi, x;
        fe_invert(zi, Z);
        fe_mul(x, X, zi);
        st = fe_isnegative(x) == (st & 1) ? kVotePass : kVoteFail;
      }
      if (st == kVotePass) {
        status_out[j] = NW_OK;
        ++passed;
        continue;
      }
    }
    src_arrays_keys src{};
    src.a = Aw; src.r = Rw; src.s = Sw; src.k = kw;
    src.ktabs = ktabs.data();
    status_out[j] = bw == -24
        ? keyset_item<24>(src, btab_lazy_entry{{BT, &SK.k.d2}, {}}, keyslot[j], kflags.data())
        : keyset_item<16>(src, btab_wide{BTW, BTW_N}, keyslot[j], kflags.data());
  }
  if (stats) { stats[0] = hotA.size(); stats[1] = checked; stats[2] = passed; stats[3] = n - passed; }
  return 0;
}

// The same slice with the comb's verdict carried to the triage (DESIGN.md 5 "Round 11"), step
// for step as the kernels take it: keyed_vote_check_ex and comb_parity_state give the item's
// state word (k_strict_keyed<true>, k_strict_keyed_inv), comb_todo_entry its to-do entry
// (k_strict_todo_list; decide = 0 is NW_STRICT_COMB_DECIDE=0), and a listed item is what
// k_strict_triage makes of the entry: strict_triage and comb_settled_status for a decided one,
// keyset_item (triage, scalars, ladder) for any other. path_out[j] says where item j's status
// came from: 0 the comb passed it, 1 settled by the triage from the comb's verdict, 2 the ladder,
// 3 rejected by the triage undecided; | 16: under a hot key, | 32: its comb sum ran. stats as
// hc_verify_strict_comb_many; dstats: items settled as NW_ERR_EQUATION, items through the ladder.
int hc_verify_strict_decided_many(const uint8_t* pks, const uint8_t* sigs, const uint8_t* k32,
                                  uint32_t n, uint64_t key_slots, int bw, uint32_t comb_min,
                                  uint32_t comb_keys, int decide, int32_t* status_out,
                                  uint8_t* path_out, uint64_t stats[4], uint64_t dstats[2]) {
  init();
  if (n == 0) return 0;
  const uint64_t slice = ((uint64_t)n + 63) & ~63ull;
  const uint32_t cap = (uint32_t)strict_keys_plan(key_slots, slice);
  std::vector<uint32_t> keyslot(n), slots(cap), kflags(cap), uses(cap), hotidx(cap, kNoKey);
  std::vector<ge_cached_pk> ktabs(8 * (size_t)cap);
  std::vector<uint32_t> pkw(8 * (size_t)n);
  memcpy(pkw.data(), pks, 32 * (size_t)n);
  uint32_t nkeys = 0;
  for (uint32_t j = 0; j < n; ++j) {
    keyslot[j] = cap ? keyset_probe(slots.data(), cap, cap / 2, &nkeys, pkw.data(), 0, j,
                                    plain_atomics{})
                     : kNoSlot;
    if (keyslot[j] != kNoSlot && comb_sampled(j)) uses[keyslot[j]] += kCombSample;
  }
  for (uint32_t s = 0; s < cap; ++s)
    keyset_build(slots.data(), s, pkw.data(), 0, SK, kflags.data(), ktabs.data());
  const uint64_t hot_cap = comb_min ? std::min<uint64_t>(comb_keys, slice / comb_min) : 0;
  std::vector<ge> hotA;
  for (uint32_t s = 0; s < cap && hotA.size() < hot_cap; ++s) {
    if (slots[s] == 0 || !comb_key_hot(uses[s], comb_min, kflags[s])) continue;
    ge A;
    if (!ge_frombytes(A, pkw.data() + 8 * (size_t)(slots[s] - 1), K)) return -2;
    hotidx[s] = (uint32_t)hotA.size();
    hotA.push_back(A);
  }
  uint64_t checked = 0, passed = 0, settled = 0, ladder = 0;
  const keyspec ks8 = keyspec_for(8);
  for (uint32_t j = 0; j < n; ++j) {
    uint32_t Aw[8], Rw[8], Sw[8], kw[8];
    load8(Aw, pks + 32 * (size_t)j); load8(Rw, sigs + 64 * (size_t)j);
    load8(Sw, sigs + 64 * (size_t)j + 32); load8(kw, k32 + 32 * (size_t)j);
    const uint32_t h = keyslot[j] != kNoSlot ? hotidx[keyslot[j]] : kNoKey;
    // the state word: no hot key in the slice leaves the whole slice to the triage, unlisted
    uint32_t state = kVoteFail;
    uint8_t where = 0;
    if (h != kNoKey) {
      ++checked;
      where |= 16;
      const strict_src_arrays src{Aw, Rw, Sw, kw};
      fe X, Z;
      state = keyed_vote_check_ex(src, SK, bcomb_lazy{BT, &SK.k.d2},
                                  keytab_lazy{&hotA[h], &SK.k.d2, ks8}, kKeyDecoded, X, Z);
      if (state != kVoteFail) where |= 32;
      if (state >= kVotePending) {
        fe zi, x;
        fe_invert(zi, Z);
        fe_mul(x, X, zi);
        state = comb_parity_state(fe_isnegative(x) == (state & 1));
      }
      if (state == kVotePass) {
        status_out[j] = NW_OK;
        if (path_out) path_out[j] = where;
        ++passed;
        continue;
      }
    }
    const uint32_t entry = hotA.empty() ? j : comb_todo_entry(j, state, decide != 0);
    src_arrays_keys src{};
    src.a = Aw; src.r = Rw; src.s = Sw; src.k = kw;
    src.ktabs = ktabs.data();
    const uint32_t slot = keyslot[comb_todo_item(entry)];
    if (entry & kTodoDecided) {
      const int st = strict_triage(static_cast<const strict_src_arrays&>(src), SK, src.xa, src.xr,
                                   slot != kNoSlot ? kflags[slot] : kNoSlot,
                                   [](bool b) { return b; });
      status_out[j] = comb_settled_status(st);
      settled += st == NW_OK;
      where |= 1;
    } else {
      bool laddered = false;
      status_out[j] = bw == -24
          ? keyset_item<24>(src, btab_lazy_entry{{BT, &SK.k.d2}, {}}, slot, kflags.data(), &laddered)
          : keyset_item<16>(src, btab_wide{BTW, BTW_N}, slot, kflags.data(), &laddered);
      ladder += laddered;
      where |= laddered ? 2 : 3;
    }
    if (path_out) path_out[j] = where;
  }
  if (stats) { stats[0] = hotA.size(); stats[1] = checked; stats[2] = passed; stats[3] = n - passed; }
  if (dstats) { dstats[0] = settled; dstats[1] = ladder; }
  return 0;
}

// The registry of registered signers alone (nw_strict.hpp signers_hash_build / signers_lookup):
// the host-built table for n distinct keys, then rows_out[i] = the registry row of probe i or
// kNoKey. Returns the table's capacity, 0 when no table holds the keys, -1 when n > max_keys
// (NW_STRICT_SIGNERS_MAX). slots_out (optional, cap words when the caller sized it from a first
// call): the table itself.
int64_t hc_signers_table(const uint8_t* keys, uint32_t n, uint64_t max_keys, const uint8_t* probes,
                         uint32_t nprobes, uint32_t* rows_out, uint32_t* slots_out) {
  if (n > max_keys) return -1;
  std::vector<uint32_t> kw(8 * (size_t)n), slots;
  if (n) memcpy(kw.data(), keys, 32 * (size_t)n);
  const uint32_t cap = signers_hash_build(kw.data(), n, slots);
  if (cap == 0) return 0;
  const signers_view sv{kw.data(), slots.data(), n ? cap : 0u};
  for (uint32_t i = 0; i < nprobes; ++i) {
    uint32_t w[8];
    load8(w, probes + 32 * (size_t)i);
    rows_out[i] = signers_lookup(sv, w);
  }
  if (slots_out) memcpy(slots_out, slots.data(), 4 * (size_t)cap);
  return (int64_t)cap;
}

// A slice the way launch_verify_strict runs it with registered signers (DESIGN.md 5
// "Round 10"): hc_verify_strict_comb_many's sequence with the registry of the nreg distinct keys
// at reg: the host-built hash table, the match of every slot of the slice's key set
// (k_strict_signers_match), the selection over one index space (registry rows first, then the
// call-local tables; a matched slot takes no ticket), the keyed check with either table, and
// the leftovers through keyset_item. The path runs even when hot_cap is 0 (n < comb_min).
// stats: as hc_verify_strict_comb_many (stats[0]: call-local tables only); sstats: registered
// keys matched, items checked under them, items passed under them.
int hc_verify_strict_signers_many(const uint8_t* pks, const uint8_t* sigs, const uint8_t* k32,
                                  uint32_t n, uint64_t key_slots, int bw, uint32_t comb_min,
                                  uint32_t comb_keys, const uint8_t* reg, uint32_t nreg,
                                  int32_t* status_out, uint64_t stats[4], uint64_t sstats[3]) {
  init();
  if (n == 0) return 0;
  // the registry: keys, hash table, flags and points (the device's tables, computed lazily)
  std::vector<uint32_t> rkeys(8 * (size_t)nreg), rslots, rok(nreg);
  if (nreg) memcpy(rkeys.data(), reg, 32 * (size_t)nreg);
  const uint32_t rcap = signers_hash_build(rkeys.data(), nreg, rslots);
  if (rcap == 0) return -3;
  const signers_view sv{rkeys.data(), rslots.data(), nreg ? rcap : 0u};
  std::vector<ge> regA(nreg);
  for (uint32_t r = 0; r < nreg; ++r) {
    const bool dec = ge_frombytes(regA[r], rkeys.data() + 8 * (size_t)r, K);
    rok[r] = (dec ? kKeyDecoded : 0u) | (dec && ge_is_small_order(regA[r]) ? kKeySmall : 0u);
  }
  const uint64_t slice = ((uint64_t)n + 63) & ~63ull;
  const uint32_t cap = (uint32_t)strict_keys_plan(key_slots, slice);
  std::vector<uint32_t> keyslot(n), slots(cap), kflags(cap), uses(cap), hotidx(cap, kNoKey);
  std::vector<ge_cached_pk> ktabs(8 * (size_t)cap);
  std::vector<uint32_t> pkw(8 * (size_t)n);
  memcpy(pkw.data(), pks, 32 * (size_t)n);
  uint32_t nkeys = 0;
  for (uint32_t j = 0; j < n; ++j) {
    keyslot[j] = cap ? keyset_probe(slots.data(), cap, cap / 2, &nkeys, pkw.data(), 0, j,
                                    plain_atomics{})
                     : kNoSlot;
    if (keyslot[j] != kNoSlot && comb_sampled(j)) uses[keyslot[j]] += kCombSample;
  }
  for (uint32_t s = 0; s < cap; ++s)
    keyset_build(slots.data(), s, pkw.data(), 0, SK, kflags.data(), ktabs.data());
  const bool on = comb_min != 0 && cap != 0;
  const uint64_t hot_cap = on ? std::min<uint64_t>(comb_keys, slice / comb_min) : 0;
  std::vector<ge> hotA;
  uint64_t matched = 0;
  for (uint32_t s = 0; on && s < cap; ++s) {
    if (slots[s] == 0) continue;
    const uint32_t* key = pkw.data() + 8 * (size_t)(slots[s] - 1);
    uint32_t row = kNoKey;
    if (nreg && comb_key_hot(0, 0, kflags[s])) row = signers_lookup(sv, key);
    if (row != kNoKey) {
      hotidx[s] = row;
      ++matched;
    } else if (hotA.size() < hot_cap && comb_key_hot(uses[s], comb_min, kflags[s])) {
      ge A;
      if (!ge_frombytes(A, key, K)) return -2;
      hotidx[s] = nreg + (uint32_t)hotA.size();
      hotA.push_back(A);
    }
  }
  uint64_t checked = 0, passed = 0, rchecked = 0, rpassed = 0;
  const keyspec ks8 = keyspec_for(8);
  for (uint32_t j = 0; j < n; ++j) {
    uint32_t Aw[8], Rw[8], Sw[8], kw[8];
    load8(Aw, pks + 32 * (size_t)j); load8(Rw, sigs + 64 * (size_t)j);
    load8(Sw, sigs + 64 * (size_t)j + 32); load8(kw, k32 + 32 * (size_t)j);
    const uint32_t h = keyslot[j] != kNoSlot ? hotidx[keyslot[j]] : kNoKey;
    if (h != kNoKey) {
      const bool isreg = h < nreg;
      ++checked;
      rchecked += isreg;
      const strict_src_arrays src{Aw, Rw, Sw, kw};
      fe X, Z;
      uint32_t st = keyed_vote_check(src, SK, bcomb_lazy{BT, &SK.k.d2},
                                     keytab_lazy{isreg ? &regA[h] : &hotA[h - nreg], &SK.k.d2, ks8},
                                     isreg ? rok[h] : kKeyDecoded, X, Z);
      if (st >= kVotePending) {
        fe zi, x;
        fe_invert(zi, Z);
        fe_mul(x, X, zi);
        st = fe_isnegative(x) == (st & 1) ? kVotePass : kVoteFail;
      }
      if (st == kVotePass) {
        status_out[j] = NW_OK;
        ++passed;
        rpassed += isreg;
        continue;
      }
    }
    src_arrays_keys src{};
    src.a = Aw; src.r = Rw; src.s = Sw; src.k = kw;
    src.ktabs = ktabs.data();
    status_out[j] = bw == -24
        ? keyset_item<24>(src, btab_lazy_entry{{BT, &SK.k.d2}, {}}, keyslot[j], kflags.data())
        : keyset_item<16>(src, btab_wide{BTW, BTW_N}, keyslot[j], kflags.data());
  }
  if (stats) { stats[0] = hotA.size(); stats[1] = checked; stats[2] = passed; stats[3] = n - passed; }
  if (sstats) { sstats[0] = matched; sstats[1] = rchecked; sstats[2] = rpassed; }
  return 0;
}

// Signature::verify_batch under the registered signers, as launch_batch_signers runs a call
// (DESIGN.md 5 "Round 12"): the registry of the nreg distinct keys at reg (host-built hash table,
// the `ok` words of the strict launches, lambda in a word array of its own), every vote through
// batch_signers_vote (lookup, flags with lambda, keyed_vote_check over the key's lazily computed
// 8-bit tables; k32 = the vote's SHA-512(R || A || digest of its batch) mod l), a pending vote's
// parity by one inversion, a failing vote's store into its batch's word, and the four counters.
// offsets: nbatches + 1 values from 0. settled_out[b] = 1 for a batch all of whose votes passed
// (an empty one included), lam_out (optional, nreg words) = the registry's lambda array,
// state_out (optional, one word per vote) = kVotePass / kVoteFail. Returns 0, -3 when no hash
// table holds the keys.
int hc_batch_signers_many(const uint8_t* reg, uint32_t nreg, const uint8_t* pks,
                          const uint8_t* sigs, const uint8_t* k32, const uint64_t* offsets,
                          uint32_t nbatches, uint32_t* settled_out, uint32_t* lam_out,
                          uint32_t* state_out, uint64_t stats[4]) {
  init();
  std::vector<uint32_t> rkeys(8 * (size_t)nreg), rslots, rok(nreg), rlam(nreg);
  if (nreg) memcpy(rkeys.data(), reg, 32 * (size_t)nreg);
  const uint32_t rcap = signers_hash_build(rkeys.data(), nreg, rslots);
  if (rcap == 0) return -3;
  const signers_view sv{rkeys.data(), rslots.data(), nreg ? rcap : 0u};
  std::vector<ge> regA(nreg);
  for (uint32_t r = 0; r < nreg; ++r) {
    const bool dec = ge_frombytes(regA[r], rkeys.data() + 8 * (size_t)r, K);
    rok[r] = (dec ? kKeyDecoded : 0u) | (dec && ge_is_small_order(regA[r]) ? kKeySmall : 0u);
    rlam[r] = dec ? key_lambda(regA[r], L_W, K.d2, torsion()) : 0u;
    if (lam_out) lam_out[r] = rlam[r];
  }
  const keyspec ks8 = keyspec_for(8);
  uint64_t ctr[4] = {0, 0, 0, 0};
  for (uint32_t b = 0; b < nbatches; ++b) settled_out[b] = 1u;
  for (uint32_t b = 0; b < nbatches; ++b) {
    for (uint64_t j = offsets[b]; j < offsets[b + 1]; ++j) {
      uint32_t Aw[8], Rw[8], Sw[8], kw[8];
      load8(Aw, pks + 32 * j); load8(Rw, sigs + 64 * j);
      load8(Sw, sigs + 64 * j + 32); load8(kw, k32 + 32 * j);
      const strict_src_arrays src{Aw, Rw, Sw, kw};
      fe X, Z;
      uint32_t st = batch_signers_vote(
          src, SK, bcomb_lazy{BT, &SK.k.d2}, sv, rok.data(), rlam.data(),
          [&](uint32_t row) { return keytab_lazy{&regA[row], &SK.k.d2, ks8}; }, X, Z);
      if (st >= kVotePending) {
        fe zi, x;
        fe_invert(zi, Z);
        fe_mul(x, X, zi);
        st = fe_isnegative(x) == (st & 1) ? kVotePass : kVoteFail;
      }
      if (st != kVotePass) settled_out[b] = 0u;
      if (state_out) state_out[j] = st;
      ++ctr[st == kVotePass ? kBsVotesPassed : kBsVotesNot];
    }
  }
  for (uint32_t b = 0; b < nbatches; ++b) ++ctr[settled_out[b] ? kBsSettled : kBsSentOn];
  if (stats) memcpy(stats, ctr, sizeof(ctr));
  return 0;
}

// k's digits at comb width w (key_recode / key_digit): digits[t], t < ntab; returns ntab.
int hc_key_digits(const uint8_t k32[32], int w, int32_t digits[32]) {
  const keyspec ks = keyspec_for((uint32_t)w);
  if (ks.W != (uint32_t)w) return -1;
  sc k;
  load8(k.w, k32);
  uint32_t kd[8];
  key_recode(kd, k, ks);
  for (uint32_t t = 0; t < ks.ntab; ++t) digits[t] = key_digit(kd, (int)t, ks);
  return (int)ks.ntab;
}

// The documented hash of a key (nw_strict.hpp keyset_hash), for the tests' numpy restatement.
uint32_t hc_keyset_hash(const uint8_t pk[32]) {
  uint32_t w[8];
  load8(w, pk);
  return keyset_hash(w);
}

// Entry j of the wide B table half h (ypx || ymx || xy2d as 30 limbs), for the table test.
void hc_wide_btab_entry(int h, uint32_t j, uint32_t out[30]) {
  init();
  memcpy(out, &BTW[(h ? BTW_N : 0u) + j].n, 120);
}

// The field (hc_fe_ops) and point (hc_ge_ops) routines on raw limbs (tools/limb_ops.hpp: the
// operation codes and the 40-word operand layout), n cases of one operation per call. No
// fe_frombytes in front, so the limbs arrive exactly as given: at their bounds, uncarried,
// non-canonical (tests/test_field_limbs_cpu.py). Returns 0, or -1 for an operation code the
// entry does not serve.
int hc_fe_ops(int op, uint32_t n, const uint32_t* A, const uint32_t* B, const int32_t* k,
              uint32_t* out) {
  if (op < 0 || op >= OP_GE_DBL) return -1;
  for (uint32_t i = 0; i < n; ++i)
    if (!limb_op(op, A + 40 * (size_t)i, B + 40 * (size_t)i, k[i], out + 40 * (size_t)i)) return -1;
  return 0;
}
int hc_ge_ops(int op, uint32_t n, const uint32_t* A, const uint32_t* B, const int32_t* k,
              uint32_t* out) {
  if (op < OP_GE_DBL) return -1;
  for (uint32_t i = 0; i < n; ++i)
    if (!limb_op(op, A + 40 * (size_t)i, B + 40 * (size_t)i, k[i], out + 40 * (size_t)i)) return -1;
  return 0;
}

// The scalar layer and the scalar phase on raw words (tools/sc_ops.hpp: the operation codes and
// the 24-word input / 40-word output layout), n cases of one operation per call
// (tests/test_sc_ops_cpu.py). out is zeroed first. Returns 0, or -1 for an operation code or a
// key width the dispatcher does not serve.
int hc_sc_ops(int op, uint32_t n, const uint32_t* in, const int32_t* k, uint32_t* out) {
  if (op < 0 || op >= SC_N) return -1;
  memset(out, 0, 4 * (size_t)kScOut * n);
  for (uint32_t i = 0; i < n; ++i)
    if (!sc_op(op, in + kScIn * (size_t)i, k[i], out + kScOut * (size_t)i)) return -1;
  return 0;
}

// The two regions of a two-pass strict launch (nw_strict_layout.hpp), for
// tests/test_strict_layout_cpu.py: every offset and the bytes of strict_region_plan (7 values),
// then of comb_region_plan with the 8-bit tables of hot_cap keys (8; the tables' bytes as
// nw_batch.hip key_tables_bytes gives them), then the offsetof of every field of triage_block_t
// and its size (5) and of comb_block_t and its size (13). Returns the number of values written.
int hc_strict_layout(uint64_t slice, uint64_t key_slots, uint64_t hot_cap, uint64_t out[]) {
  const strict_region_t r = strict_region_plan(slice, key_slots);
  const keyspec ks8 = keyspec_for(8);
  const uint64_t nk = hot_cap ? hot_cap : 1;
  const comb_region_t c = comb_region_plan(
      slice, key_slots, hot_cap,
      sizeof(ge_niels_pad) * (uint64_t)ks8.tab * nk + sizeof(ge) * (2 + keyspec_tables(ks8)) * nk);
  const uint64_t v[] = {
      r.list, r.keyslot, r.block, r.slots, r.kflags, r.ktabs, r.bytes,
      c.todo, c.uses, c.hotidx, c.match, c.hotrow, c.hok, c.tabs, c.bytes,
      offsetof(triage_block_t, count), offsetof(triage_block_t, nkeys),
      offsetof(triage_block_t, keys_tabulated), offsetof(triage_block_t, with_slot),
      sizeof(triage_block_t),
      offsetof(comb_block_t, nhot), offsetof(comb_block_t, todo_count),
      offsetof(comb_block_t, nlive), offsetof(comb_block_t, hot_keys),
      offsetof(comb_block_t, checked), offsetof(comb_block_t, listed),
      offsetof(comb_block_t, matched), offsetof(comb_block_t, laddered),
      offsetof(comb_block_t, lane_checked), offsetof(comb_block_t, lane_reg_items),
      offsetof(comb_block_t, lane_reg_passed), offsetof(comb_block_t, lane_settled),
      sizeof(comb_block_t)};
  const int count = (int)(sizeof(v) / sizeof(v[0]));
  for (int i = 0; i < count; ++i) out[i] = v[i];
  return count;
}

// The key-major order's region (nw_strict_keymajor.hpp), for tests/test_strict_keymajor_cpu.py:
// every offset and the bytes of km_region_plan (5 values), the bytes cleared per launch, kKmBins
// and kKmChunk, then the offsetof of every field of km_block_t and its size (5). Returns the
// number of values written.
int hc_keymajor_layout(uint64_t slice, uint64_t out[]) {
  const km_region_t r = km_region_plan(slice);
  const uint64_t v[] = {r.hist, r.cursor, r.perm, r.pslot, r.bytes, kKmClearBytes, kKmBins, kKmChunk,
                        offsetof(km_block_t, npos), offsetof(km_block_t, placed),
                        offsetof(km_block_t, bins), offsetof(km_block_t, slices),
                        sizeof(km_block_t)};
  const int count = (int)(sizeof(v) / sizeof(v[0]));
  for (int i = 0; i < count; ++i) out[i] = v[i];
  return count;
}
// The bin of key index kk among `space` live indices (km_shift, km_bin); *shift_out = the shift.
uint32_t hc_keymajor_bin(uint32_t kk, uint32_t space, uint32_t* shift_out) {
  const uint32_t shift = km_shift(space);
  if (shift_out) *shift_out = shift;
  return km_bin(kk, space, shift);
}

}

#ifdef KEYSET_SAN_MAIN
// make keysetsan && tools/keyset_san: the key set's sizing and region planning
// (nw_kernels.h strict_keys_plan / strict_region_plan) and the probe -> build -> triage ->
// ladder sequence over that region, then the registered signers' hash table (build, lookup,
// limit), one slice through a registry and one verify_batch call under it, as a stand-alone
// program under AddressSanitizer / UBSan.
#include <stdio.h>
#include <vector>
static int san_fail(const char* what, uint64_t a, uint64_t b) {
  fprintf(stderr, "keyset_san: %s (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b);
  return 1;
}
int main() {
  const uint64_t reqs[] = {0, 1, 63, 64, 65, 1000, 65536, 1ull << 20, (1ull << 20) + 1, 1ull << 40, ~0ull};
  const uint64_t slices[] = {0, 64, 128, 1536, 196608, 1ull << 24};
  for (uint64_t rq : reqs)
    for (uint64_t sl : slices) {
      const uint64_t cap = strict_keys_plan(rq, sl);
      if (rq == 0 || sl == 0) {
        if (cap != 0) return san_fail("plan: off expected", rq, sl);
        continue;
      }
      if (cap < kKeySlotsMin || cap > kKeySlotsMax || (cap & (cap - 1)))
        return san_fail("plan: slots out of range", rq, sl);
      if (cap >= 2 * kKeySlotsMin && cap / 2 >= 4 * sl) return san_fail("plan: over the slice", rq, sl);
      if (cap / 2 >= rq && cap > kKeySlotsMin) return san_fail("plan: over the request", rq, sl);
      const strict_region_t rg = strict_region_plan(sl, cap);
      if (!(rg.list < rg.keyslot && rg.keyslot < rg.block && rg.block + kTriageBlockBytes <= rg.slots &&
            rg.slots + 4 * cap <= rg.kflags && rg.kflags + 4 * cap <= rg.ktabs &&
            rg.ktabs % 256 == 0 && rg.block % 8 == 0 && rg.bytes == rg.ktabs + kKeyTabBytes * cap))
        return san_fail("region: layout", rq, sl);
    }
  // the sequence itself: repeated keys, keys without a slot (64 slots), and the set off
  uint32_t seed = 12345;
  auto rnd = [&] { return (uint8_t)((seed = seed * 1664525u + 1013904223u) >> 24); };
  for (uint32_t n : {1u, 65u, 300u}) {
    const uint32_t nk = n < 100 ? 3 : 90;
    std::vector<uint8_t> keys(32 * nk), pks(32 * n), sigs(64 * n), ks(32 * n);
    for (auto& b : keys) b = rnd();
    for (uint32_t j = 0; j < n; ++j) {
      memcpy(&pks[32 * j], &keys[32 * (j % nk)], 32);
      for (int t = 0; t < 64; ++t) sigs[64 * j + t] = rnd();
      sigs[64 * j + 63] &= 0x0f;   // s canonical, so the items whose points decode reach the ladder
      for (int t = 0; t < 32; ++t) ks[32 * j + t] = rnd();
      ks[32 * j + 31] &= 0x0f;
    }
    std::vector<int32_t> off(n), on(n);
    uint64_t st[3];
    if (hc_verify_strict_keyset_many(pks.data(), sigs.data(), ks.data(), n, 0, -16, off.data(), nullptr, st))
      return san_fail("run (off)", n, 0);
    if (st[0] != 0 || st[1] != 0 || st[2] != n) return san_fail("stats (off)", st[1], st[2]);
    for (uint64_t slots : {64ull, 65536ull}) {
      std::vector<uint32_t> ksl(n);
      if (hc_verify_strict_keyset_many(pks.data(), sigs.data(), ks.data(), n, slots, -16, on.data(), ksl.data(), st))
        return san_fail("run (on)", n, slots);
      if (on != off) return san_fail("statuses differ", n, slots);
      if (st[1] + st[2] != n || st[0] > 32768 || st[1] == 0) return san_fail("stats (on)", st[0], st[1]);
    }
  }
  // registered signers: the hash table for a few hundred keys (every one found, strangers
  // not), then one slice through the registry: some keys registered, below and above the
  // call-local threshold, against the same slice without a registry
  {
    const uint32_t nk = 300, n = 300;
    std::vector<uint8_t> keys(32 * nk), strangers(32 * 64);
    for (auto& b : keys) b = rnd();
    for (auto& b : strangers) b = rnd();
    std::vector<uint32_t> rows(nk);
    const int64_t cap = hc_signers_table(keys.data(), nk, 8192, keys.data(), nk, rows.data(), nullptr);
    if (cap < 2 * nk || (cap & (cap - 1))) return san_fail("signers: capacity", (uint64_t)cap, nk);
    for (uint32_t r = 0; r < nk; ++r)
      if (rows[r] != r) return san_fail("signers: lookup", r, rows[r]);
    if (hc_signers_table(keys.data(), nk, 8192, strangers.data(), 64, rows.data(), nullptr) != cap)
      return san_fail("signers: capacity (again)", 0, 0);
    for (uint32_t r = 0; r < 64; ++r)
      if (rows[r] != kNoKey) return san_fail("signers: stranger found", r, rows[r]);
    if (hc_signers_table(keys.data(), 0, 8192, strangers.data(), 64, rows.data(), nullptr) <= 0)
      return san_fail("signers: empty", 0, 0);
    if (hc_signers_table(keys.data(), nk, nk - 1, nullptr, 0, nullptr, nullptr) != -1)
      return san_fail("signers: limit", 0, 0);
    std::vector<uint8_t> pks(32 * n), sigs(64 * n), ks(32 * n);
    for (uint32_t j = 0; j < n; ++j) {
      memcpy(&pks[32 * j], &keys[32 * (j % 5)], 32);
      for (int t = 0; t < 64; ++t) sigs[64 * j + t] = rnd();
      sigs[64 * j + 63] &= 0x0f;
      for (int t = 0; t < 32; ++t) ks[32 * j + t] = rnd();
      ks[32 * j + 31] &= 0x0f;
    }
    std::vector<int32_t> off(n), on(n);
    uint64_t st[4], ss[3];
    if (hc_verify_strict_signers_many(pks.data(), sigs.data(), ks.data(), n, 65536, -16, 256, 8192,
                                      nullptr, 0, off.data(), st, ss))
      return san_fail("signers: run (none)", 0, 0);
    if (ss[0] || ss[1] || ss[2] || st[1]) return san_fail("signers: stats (none)", ss[0], st[1]);
    for (uint32_t cmin : {256u, 32u}) {
      if (hc_verify_strict_signers_many(pks.data(), sigs.data(), ks.data(), n, 65536, -16, cmin, 8192,
                                        keys.data(), 3, on.data(), st, ss))
        return san_fail("signers: run", cmin, 0);
      if (on != off) return san_fail("signers: statuses differ", cmin, 0);
      if (ss[0] > 3 || ss[2] > ss[1] || ss[1] > st[1] || st[2] + st[3] != n)
        return san_fail("signers: stats", ss[0], ss[1]);
    }
  }
  // plain batches under the registry (hc_batch_signers_many): empty batches, registered and
  // unregistered signers, garbage signatures; nothing random passes, every empty batch is settled
  {
    const uint32_t nk = 6, nb = 40;
    std::vector<uint8_t> keys(32 * nk);
    for (auto& b : keys) b = rnd();
    std::vector<uint64_t> offs(nb + 1, 0);
    uint32_t empty = 0;
    for (uint32_t b = 0; b < nb; ++b) {
      const uint32_t c = rnd() % 7;
      empty += c == 0;
      offs[b + 1] = offs[b] + c;
    }
    const uint32_t n = (uint32_t)offs[nb];
    std::vector<uint8_t> pks(32 * n + 32), sigs(64 * n + 64), ks(32 * n + 32);
    for (uint32_t j = 0; j < n; ++j) {
      memcpy(&pks[32 * j], &keys[32 * (j % nk)], 32);
      for (int t = 0; t < 64; ++t) sigs[64 * j + t] = rnd();
      sigs[64 * j + 63] &= 0x0f;
      for (int t = 0; t < 32; ++t) ks[32 * j + t] = rnd();
      ks[32 * j + 31] &= 0x0f;
    }
    for (uint32_t nreg : {0u, 4u, 6u}) {
      std::vector<uint32_t> settled(nb), lam(nreg), state(n);
      uint64_t st[4];
      if (hc_batch_signers_many(keys.data(), nreg, pks.data(), sigs.data(), ks.data(), offs.data(), nb,
                                settled.data(), lam.data(), state.data(), st))
        return san_fail("batch signers: run", nreg, 0);
      if (st[0] != 0 || st[1] != n || st[2] != empty || st[2] + st[3] != nb)
        return san_fail("batch signers: stats", st[0], st[2]);
      for (uint32_t b = 0; b < nb; ++b)
        if (settled[b] != (offs[b + 1] == offs[b] ? 1u : 0u)) return san_fail("batch signers: word", b, settled[b]);
      for (uint32_t r = 0; r < nreg; ++r)
        if (lam[r] > 7) return san_fail("batch signers: lambda", r, lam[r]);
    }
  }
  printf("keyset_san ok\n");
  return 0;
}
#endif
