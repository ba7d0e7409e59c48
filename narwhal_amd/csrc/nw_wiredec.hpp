// nw_wiredec.hpp — per-frame decoder of bincode PrimaryMessage frames, written once as
// __host__ __device__ code: the kernels of nw_wire.hip run it on the device, and
// tools/wirecheck.hip compiles the same text for the CPU (tests/test_wire_device_cpu.py).
// The wire format and every accept / reject rule are nw_wire.cpp's (decode_frame), bit for
// bit; that file's header comment describes the format.
//
// Two steps per frame:
//   scan  one walk over the frame: the kind (NW_MSG_* or -1), the counts, the two key-text
//         lengths the emit needs to find every field again, and the `canonical` bit (raw
//         payload keys strictly increasing and raw parents strictly increasing, as 32-byte
//         lexicographic compares). A strictly increasing sequence has no duplicates, so for a
//         canonical frame BTreeMap / BTreeSet deserialisation changes nothing: the
//         `Hash for Header` bytes are the frame's own payload and parent bytes in place, and
//         no sort is needed. Non-canonical Header / Certificate frames (which an honest
//         sender never produces: bincode writes a BTreeMap / BTreeSet in key order) are left
//         to the host decoder, unless the caller asks for the canonicalisation below
//         (canon_*, emit_lane<true>), which sorts and de-duplicates them on the device.
//   emit  writes the item's structure-of-arrays rows as 4-byte words, cooperatively: the
//         frame's output is a list of word tasks, lane l of a group of G takes tasks l,
//         l + G, ..., so contiguous lanes write contiguous words. Every destination is
//         4-byte aligned (header bytes are 40 + 36 np + 32 nq long, every other row is a
//         multiple of 32 bytes). A record that does not fit its own frame (header_layout /
//         vote_layout) emits nothing, a certificate record whose votes do not fit (8 + 72 nv)
//         not even its header rows; the host rejects such a record before any emit runs.
//
// Memory access: frames start at arbitrary byte offsets, so the frame buffer is read as
// aligned 32-bit words plus a shift (never an unaligned wide load). The buffer `w` must be
// 4-byte aligned and readable up to the next multiple of 4 past the last frame byte; bytes
// past a frame's end are shifted or masked out and never reach a decision.
#pragma once
#include <stdint.h>

#ifndef NW_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define NW_HD __host__ __device__ inline
#else
#define NW_HD inline
#endif
#endif

namespace nw {
namespace wd {

// One frame's scan result (32 bytes; written by the scan, read by the emit and the host).
struct rec_t {
  int32_t kind;        // NW_MSG_* (0..3), -1 = does not decode, kOverCap = not scanned
  uint32_t canonical;  // 1: payload keys and parents strictly increasing (kinds 0 / 2; 1 for
                       // votes and requests, 0 when kind < 0)
  uint32_t np;         // payload entries as sent (CertificatesRequest: digests requested)
  uint32_t nq;         // parents as sent
  uint32_t nv;         // votes (certificates)
  uint32_t alen;       // key text length: the author's (header / certificate), origin's (vote)
  uint32_t vlen;       // certificate: the votes' common key text length, 0 when they differ
                       // (or there are none); vote: the author's key text length
  uint32_t reserved;   // 0
};
constexpr int32_t kOverCap = -2;   // longer than the caller's cap: the host decodes it

// Where the host placed one frame's output (16 bytes): its slot among the items of its
// kind, the start of its header bytes and of its votes. slot = kNoSlot: nothing to emit.
struct dst_t {
  uint64_t hb_off;
  uint32_t slot;
  uint32_t vote0;
};
constexpr uint32_t kNoSlot = 0xffffffffu;

// Destination arrays of one call (device pointers in the kernel). The counts are the
// capacities the emit checks every write against.
struct out_t {
  // headers (k = 0) and certificates (k = 1)
  uint8_t* hb[2];        // header bytes
  uint64_t hb_len[2];
  uint64_t* ho[2];       // n + 1 offsets
  uint32_t* pc[2];       // payload counts
  uint32_t* ids[2];      // n x 8 words
  uint32_t* sigs[2];     // n x 16 words
  uint32_t nitems[2];
  uint64_t* vo;          // certificates: n + 1 vote offsets
  uint32_t* vpk;         // nvotes x 8 words
  uint32_t* vsig;        // nvotes x 16 words
  uint32_t nvotes;
  // Vote messages
  uint32_t* v_ids;
  uint64_t* v_rounds;
  uint32_t* v_origins;
  uint32_t* v_authors;
  uint32_t* v_sigs;
  uint32_t nvmsg;
};

// ---- aligned-word reads -------------------------------------------------------------
NW_HD uint32_t rd_u8(const uint32_t* w, uint64_t a) {
  return (w[a >> 2] >> ((uint32_t)(a & 3) * 8)) & 0xffu;
}
NW_HD uint32_t rd_u32(const uint32_t* w, uint64_t a) {
  const uint32_t sh = (uint32_t)(a & 3) * 8;
  const uint32_t lo = w[a >> 2];
  if (sh == 0) return lo;
  return (lo >> sh) | (w[(a >> 2) + 1] << (32 - sh));
}
NW_HD uint64_t rd_u64(const uint32_t* w, uint64_t a) {
  return (uint64_t)rd_u32(w, a) | ((uint64_t)rd_u32(w, a + 4) << 32);
}
// The word as a big-endian number: comparing these compares the 4 bytes lexicographically.
NW_HD uint32_t bswap32(uint32_t v) {
  return (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24);
}
// memcmp(a, b, 32) < 0
NW_HD bool less32(const uint32_t* w, uint64_t a, uint64_t b) {
  for (int k = 0; k < 8; ++k) {
    const uint32_t x = rd_u32(w, a + 4 * k), y = rd_u32(w, b + 4 * k);
    if (x != y) return bswap32(x) < bswap32(y);
  }
  return false;
}

NW_HD int b64_value(uint32_t c) {
  if (c >= 'A' && c <= 'Z') return (int)c - 'A';
  if (c >= 'a' && c <= 'z') return (int)c - 'a' + 26;
  if (c >= '0' && c <= '9') return (int)c - '0' + 52;
  if (c == '+') return 62;
  if (c == '/') return 63;
  return -1;
}

// base64 0.13 STANDARD over the text at absolute byte a, len bytes: validates the whole
// string as nw_wire.cpp's b64_decode32 does (padding optional, padded input in whole quads,
// a lone trailing symbol rejected, non-zero trailing bits rejected) and returns whether it
// decodes to at least 32 bytes. Nothing is written: the emit decodes the first 32 bytes.
NW_HD bool b64_check32(const uint32_t* w, uint64_t a, uint64_t len) {
  uint64_t end = len;
  int pad = 0;
  while (end > 0 && pad < 2 && rd_u8(w, a + end - 1) == '=') {
    --end;
    ++pad;
  }
  if (pad && (len % 4) != 0) return false;
  if (end % 4 == 1) return false;
  if (pad && (int)(end % 4) + pad != 4) return false;
  uint32_t acc = 0;
  int bits = 0;
  uint64_t nout = 0;
  uint64_t ci = ~(uint64_t)0;
  uint32_t cw = 0;
  for (uint64_t i = 0; i < end; ++i) {
    const uint64_t p = a + i;
    if ((p >> 2) != ci) {   // one aligned load per four symbols
      ci = p >> 2;
      cw = w[ci];
    }
    const int v = b64_value((cw >> ((uint32_t)(p & 3) * 8)) & 0xffu);
    if (v < 0) return false;
    acc = (acc << 6) | (uint32_t)v;
    bits += 6;
    if (bits >= 8) {
      bits -= 8;
      ++nout;
      acc &= (1u << bits) - 1;
    }
  }
  return acc == 0 && nout >= 32;
}

// Decoded bytes 4 j .. 4 j + 3 (j < 8) of a key text that passed b64_check32, as one
// little-endian word: byte b comes from symbols 4 (b / 3) + b % 3 and the next one.
NW_HD uint32_t b64_word(const uint32_t* w, uint64_t a, uint32_t j) {
  uint32_t out = 0;
  for (uint32_t k = 0; k < 4; ++k) {
    const uint32_t b = 4 * j + k, q = b / 3, r = b % 3;
    const uint32_t c0 = (uint32_t)b64_value(rd_u8(w, a + 4 * q + r));
    const uint32_t c1 = (uint32_t)b64_value(rd_u8(w, a + 4 * q + r + 1));
    out |= (((c0 << (2 + 2 * r)) | (c1 >> (4 - 2 * r))) & 0xffu) << (8 * k);
  }
  return out;
}

// ---- scan ---------------------------------------------------------------------------
// A cursor over frame bytes [off, off + len): take() is nw_wire.cpp's Reader::take.
struct cur_t {
  const uint32_t* w;
  uint64_t off, len, pos;
  bool ok;
};
NW_HD uint64_t cur_take(cur_t& c, uint64_t k) {   // absolute address of the k bytes taken
  if (!c.ok || k > c.len - c.pos) {
    c.ok = false;
    return 0;
  }
  const uint64_t a = c.off + c.pos;
  c.pos += k;
  return a;
}
NW_HD uint64_t cur_u64(cur_t& c) {
  const uint64_t a = cur_take(c, 8);
  return c.ok ? rd_u64(c.w, a) : 0;
}
// A sequence length that cannot exceed the remaining bytes at elem bytes per element: by
// division, never by a product that can wrap.
NW_HD uint64_t cur_len(cur_t& c, uint64_t elem) {
  const uint64_t v = cur_u64(c);
  if (c.ok && v > (c.len - c.pos) / elem) c.ok = false;
  return c.ok ? v : 0;
}
// A PublicKey: u64 length, base64 text decoding to >= 32 bytes. *tlen = the text length.
NW_HD bool cur_pk(cur_t& c, uint64_t* tlen) {
  const uint64_t L = cur_len(c, 1);
  const uint64_t a = cur_take(c, L);
  if (!c.ok) return false;
  if (!b64_check32(c.w, a, L)) return (c.ok = false);
  *tlen = L;
  return true;
}

// Scans frame bytes [off, off + len) of the word buffer w. len < 2^32 (the callers cap it).
NW_HD rec_t scan(const uint32_t* w, uint64_t off, uint64_t len) {
  rec_t r{-1, 0, 0, 0, 0, 0, 0, 0};
  cur_t c{w, off, len, 0, true};
  const uint64_t va = cur_take(c, 4);
  if (!c.ok) return r;
  const uint32_t variant = rd_u32(w, va);
  if (variant > 3) return r;
  if (variant == 0 || variant == 2) {
    uint64_t alen = 0;
    if (!cur_pk(c, &alen)) return r;
    (void)cur_take(c, 8);   // round
    const uint64_t np = cur_len(c, 36);
    const uint64_t pay = cur_take(c, 36 * np);
    const uint64_t nq = cur_len(c, 32);
    const uint64_t par = cur_take(c, 32 * nq);
    (void)cur_take(c, 32 + 64);   // id, signature
    if (!c.ok) return r;
    uint64_t nv = 0, vlen = 0;
    if (variant == 2) {
      nv = cur_len(c, 72);   // each vote >= 8-byte length + 64-byte signature
      bool same = true;
      for (uint64_t v = 0; v < nv && c.ok; ++v) {
        uint64_t L = 0;
        if (!cur_pk(c, &L)) break;
        (void)cur_take(c, 64);
        if (v == 0) vlen = L;
        else if (L != vlen) same = false;
      }
      if (!c.ok) return r;
      if (!same) vlen = 0;
    }
    bool canon = true;
    for (uint64_t i = 1; i < np && canon; ++i) canon = less32(w, pay + 36 * (i - 1), pay + 36 * i);
    for (uint64_t i = 1; i < nq && canon; ++i) canon = less32(w, par + 32 * (i - 1), par + 32 * i);
    r.kind = (int32_t)variant;
    r.canonical = canon ? 1u : 0u;
    r.np = (uint32_t)np;
    r.nq = (uint32_t)nq;
    r.nv = (uint32_t)nv;
    r.alen = (uint32_t)alen;
    r.vlen = (uint32_t)vlen;
    return r;
  }
  if (variant == 1) {
    uint64_t lo = 0, la = 0;
    (void)cur_take(c, 32 + 8);   // id, round
    if (!c.ok || !cur_pk(c, &lo) || !cur_pk(c, &la)) return r;
    (void)cur_take(c, 64);
    if (!c.ok) return r;
    r.kind = 1;
    r.canonical = 1;
    r.alen = (uint32_t)lo;
    r.vlen = (uint32_t)la;
    return r;
  }
  // CertificatesRequest(Vec<Digest>, PublicKey): decoded for well-formedness only.
  const uint64_t nd = cur_len(c, 32);
  (void)cur_take(c, 32 * nd);
  uint64_t L = 0;
  if (!c.ok || !cur_pk(c, &L)) return r;
  r.kind = 3;
  r.canonical = 1;
  r.np = (uint32_t)nd;
  return r;
}

// ---- frame layout -------------------------------------------------------------------
// The only place that knows the field offsets: where a record says its frame's fields are
// (absolute byte addresses) and whether it fits its own frame [off, off + len) (ok). The emit,
// canon_begin and the host's placement (nw_wireplace.hpp) ask here. Sums in 64 bits: no wrap.
// variant 4 | author: len 8, text | round 8 | np 8 | payload 36 each | nq 8 | parents 32 each
// | id 32 | signature 64 | (certificate) nv 8 | votes: len 8, text, signature 64
struct hdr_layout_t {   // author text, round, payload, parents, id, end of the signature, votes
  uint64_t at, rnd, pay, par, idp, hend, vts; bool ok;
};
NW_HD hdr_layout_t header_layout(uint64_t off, uint64_t len, const rec_t& r) {
  const uint64_t pb = 36 * (uint64_t)r.np, qb = 32 * (uint64_t)r.nq, at = off + 12,
                 rnd = at + r.alen, pay = rnd + 16, par = pay + pb + 8, idp = par + qb;
  return {at, rnd, pay, par, idp, idp + 96, idp + 96 + 8,
          132 + (uint64_t)r.alen + pb + qb + (r.kind == 2 ? 8 + 72 * (uint64_t)r.nv : 0) <= len};
}
// variant 4 | id 32 | round 8 | origin: len 8, text | author: len 8, text | signature 64
struct vote_layout_t {   // id, round, origin text, author text, signature; the record fits
  uint64_t id, rnd, ot, at, sg; bool ok;
};
NW_HD vote_layout_t vote_layout(uint64_t off, uint64_t len, const rec_t& r) {
  const uint64_t ot = off + 52, at = ot + r.alen + 8;
  return {off + 4, off + 36, ot, at, at + r.vlen, 124 + (uint64_t)r.alen + r.vlen <= len};
}

// Bytes of the `Hash for Header` input (np, nq: raw counts, or a canonicalised frame's kept ones).
NW_HD uint64_t header_len(uint32_t np, uint32_t nq) { return 40 + 36 * (uint64_t)np + 32 * (uint64_t)nq; }

// ---- canonicalisation of non-canonical Header / Certificate frames --------------------
// BTreeMap / BTreeSet deserialisation of a frame whose payload keys or parents are not
// strictly increasing as sent: sort each section by key (32-byte lexicographic, unsigned),
// keep one entry per key, in the payload the one that comes last in wire order (its worker
// id wins). Nothing is moved: the result is an order list, one index per kept entry that
// says which wire entry supplies that output position, and the emit reads the frame through
// it. A group of lanes works on one frame, in phases with a barrier between them that the
// caller supplies (the kernel: __syncthreads(); the CPU check: a loop over the lanes per
// phase):
//   canon_stage  the keys of both sections go into `keys`, 8 words per entry, each word
//                byte-swapped, so that the lexicographic compare is an unsigned word compare,
//                most significant word first;
//   canon_mark   entry i is dropped if a later entry of its section has the same key;
//   canon_rank   a kept entry's output position is the number of kept entries of its section
//                with a smaller key; one lane per section counts the kept entries.
// Lane l of L takes entries l, l + L, ...; in the walks over j every lane reads the same
// key, a broadcast in LDS. O(n^2 / L) compares of at most 8 words, n <= kCanonMax.
//
// The order list of the frame at byte offset off starts at word ceil(off / 32) of a scratch
// of ceil(total / 32) + 1 words (total = all frames' bytes): payload positions at [0, np_u),
// parent positions at [np, np + nq_u), np the raw payload count, so that no phase needs a
// count that another lane of the same phase produces. A frame holds 132 bytes besides its
// entries and every entry takes at least 32, so len >= 32 (np + nq) + 132 and
// ceil(off / 32) + np + nq <= ceil(off / 32) + floor(len / 32) <= ceil((off + len) / 32): the
// lists of two frames cannot overlap and the last one ends inside the scratch, for any
// input. Every write is checked against the scratch's capacity all the same.
constexpr uint32_t kCanonMax = 1024;   // entries per frame (payload + parents) the device sorts
enum : uint32_t {
  kCanonNone = 0,   // not applicable: not a Header / Certificate, does not decode, or canonical
  kCanonDone = 1,   // canonicalised: np_u / nq_u and the order list are valid
  kCanonOver = 2,   // more than kCanonMax entries: the host decodes it
};
// One frame's result, beside its rec_t (16 bytes).
struct canon_t {
  uint32_t np_u, nq_u;   // kept payload entries, kept parents
  uint32_t state;        // kCanon*
  uint32_t reserved;     // 0
};
// What the phases of one frame share.
struct canon_job_t {
  const uint32_t* w;
  uint64_t pay, par;     // absolute byte address of the first payload entry / first parent
  uint32_t np, nq;       // raw counts
  uint64_t list, cap;    // first word of the frame's order list, words in the scratch
};

NW_HD uint64_t canon_list_words(uint64_t total) { return (total + 31) / 32 + 1; }

// The state of frame [off, off + len) with scan result r; for kCanonDone, *jb is filled in.
NW_HD uint32_t canon_begin(const uint32_t* w, uint64_t off, uint64_t len, const rec_t& r,
                           uint64_t order_cap, canon_job_t* jb) {
  if ((r.kind != 0 && r.kind != 2) || r.canonical) return kCanonNone;
  // Deliberately h.hend, not h.ok: only the part this reads, up to the signature, as before
  // the layout functions. With the votes' term the kernel's loops land elsewhere, which cost
  // k_wire_canon<256> 3 to 8 % on frames of 1,018 entries (profiles/wire03; it may differ with
  // another compiler). The placement rejects a record whose votes do not fit.
  const hdr_layout_t h = header_layout(off, len, r);
  if (h.hend > off + len) return kCanonNone;   // (not the scan's record)
  if ((uint64_t)r.np + r.nq > kCanonMax) return kCanonOver;
  *jb = canon_job_t{w, h.pay, h.par, r.np, r.nq, (off + 31) / 32, order_cap};
  return kCanonDone;
}

// keys: 8 (np + nq) words.
NW_HD void canon_stage(uint32_t lane, uint32_t lanes, const canon_job_t& jb, uint32_t* keys) {
  const uint32_t T = 8 * (jb.np + jb.nq);
  for (uint32_t t = lane; t < T; t += lanes) {
    const uint32_t e = t / 8, k = t % 8;
    const uint64_t a = e < jb.np ? jb.pay + 36 * (uint64_t)e : jb.par + 32 * (uint64_t)(e - jb.np);
    keys[t] = bswap32(rd_u32(jb.w, a + 4 * k));
  }
}

// -1 / 0 / 1: the staged key a against the key held in k[8].
NW_HD int canon_cmp(const uint32_t* a, const uint32_t* k) {
  for (int i = 0; i < 8; ++i)
    if (a[i] != k[i]) return a[i] < k[i] ? -1 : 1;
  return 0;
}

// kept: np + nq words, 1 = the entry survives.
NW_HD void canon_mark(uint32_t lane, uint32_t lanes, const canon_job_t& jb, const uint32_t* keys,
                      uint32_t* kept) {
  const uint32_t n = jb.np + jb.nq;
  for (uint32_t i = lane; i < n; i += lanes) {
    const uint32_t end = i < jb.np ? jb.np : n;
    uint32_t k[8];
    for (int x = 0; x < 8; ++x) k[x] = keys[8 * i + x];
    uint32_t keep = 1;
    for (uint32_t j = i + 1; j < end && keep; ++j)
      if (canon_cmp(keys + 8 * j, k) == 0) keep = 0;
    kept[i] = keep;
  }
}

// Writes the order list and *out (state kCanonDone).
NW_HD void canon_rank(uint32_t lane, uint32_t lanes, const canon_job_t& jb, const uint32_t* keys,
                      const uint32_t* kept, uint32_t* order, canon_t* out) {
  const uint32_t n = jb.np + jb.nq;
  for (uint32_t i = lane; i < n; i += lanes) {
    if (!kept[i]) continue;
    const uint32_t beg = i < jb.np ? 0 : jb.np, end = i < jb.np ? jb.np : n;
    uint32_t k[8];
    for (int x = 0; x < 8; ++x) k[x] = keys[8 * i + x];
    uint32_t pos = 0;
    for (uint32_t j = beg; j < end; ++j)
      if (kept[j] && canon_cmp(keys + 8 * j, k) < 0) ++pos;
    const uint64_t at = jb.list + beg + pos;   // beg + pos < np + nq
    if (at < jb.cap) order[at] = i - beg;
  }
  // the counts: one lane per section (the same lane when there is only one)
  if (lane == 0) {
    uint32_t c = 0;
    for (uint32_t j = 0; j < jb.np; ++j) c += kept[j];
    out->np_u = c;
    out->state = kCanonDone;
    out->reserved = 0;
  }
  if (lane == (lanes > 1 ? 1u : 0u)) {
    uint32_t c = 0;
    for (uint32_t j = jb.np; j < n; ++j) c += kept[j];
    out->nq_u = c;
  }
}

// ---- emit ---------------------------------------------------------------------------
// The Header / Certificate rows of emit_lane. kSorted: the frame's canon_t c says kCanonDone,
// and its header bytes take their payload entries and parents through the order list (header
// word t of the payload range is word (t - 10) % 9 of wire entry order[(t - 10) / 9], parents
// likewise, 8 words each; an index not below its section's raw count writes nothing) and
// their length and payload count from the kept counts; the id, the signature and the votes
// are found with the raw counts. An instance per value, so that no word pays for the choice.
template <bool kSorted>
NW_HD void emit_header(const uint32_t* w, uint64_t off, uint64_t len, const rec_t& r,
                       const canon_t* c, const uint32_t* order, uint64_t order_cap,
                       const dst_t& d, const out_t& o, uint32_t lane, uint32_t G) {
  const uint64_t list = (off + 31) / 32;
  if (kSorted && (c->state != kCanonDone || c->np_u > r.np || c->nq_u > r.nq ||
                  list + r.np + r.nq > order_cap))
    return;
  const uint32_t* ord = kSorted ? order + list : nullptr;
  const uint32_t np = kSorted ? c->np_u : r.np, nq = kSorted ? c->nq_u : r.nq;   // of the header bytes
  const int k = r.kind == 2 ? 1 : 0;
  const uint64_t hl = header_len(np, nq);
  if (d.slot >= o.nitems[k] || d.hb_off > o.hb_len[k] || hl > o.hb_len[k] - d.hb_off) return;
  if (k && ((uint64_t)d.vote0 + r.nv > o.nvotes)) return;
  const hdr_layout_t f = header_layout(off, len, r);
  if (!f.ok) return;
  if (lane == 0) {
    o.ho[k][d.slot] = d.hb_off;
    o.ho[k][(uint64_t)d.slot + 1] = d.hb_off + hl;   // the next frame writes the same value
    o.pc[k][d.slot] = np;
    if (k) {
      o.vo[d.slot] = d.vote0;
      o.vo[(uint64_t)d.slot + 1] = (uint64_t)d.vote0 + r.nv;
    }
  }
  uint32_t* hb = reinterpret_cast<uint32_t*>(o.hb[k] + d.hb_off);
  const uint32_t hw = (uint32_t)(hl / 4), pw = 10 + 9 * np;
  const uint32_t T = hw + 24 + (k ? 24 * r.nv : 0);
  // votes with differing key text lengths: this lane walks forward from vote to vote
  uint32_t wv = 0;
  uint64_t wpos = f.vts;
  for (uint32_t t = lane; t < T; t += G) {
    if (t < 8) hb[t] = b64_word(w, f.at, t);
    else if (t < 10) hb[t] = rd_u32(w, f.rnd + 4 * (t - 8));
    else if (t < pw) {
      if (kSorted) {
        const uint32_t e = ord[(t - 10) / 9];
        if (e < r.np) hb[t] = rd_u32(w, f.pay + 36 * (uint64_t)e + 4 * ((t - 10) % 9));
      } else hb[t] = rd_u32(w, f.pay + 4 * (uint64_t)(t - 10));
    } else if (t < hw) {
      if (kSorted) {
        const uint32_t e = ord[r.np + (t - pw) / 8];
        if (e < r.nq) hb[t] = rd_u32(w, f.par + 32 * (uint64_t)e + 4 * ((t - pw) % 8));
      } else hb[t] = rd_u32(w, f.par + 4 * (uint64_t)(t - pw));
    } else if (t < hw + 8) o.ids[k][8 * (uint64_t)d.slot + (t - hw)] = rd_u32(w, f.idp + 4 * (t - hw));
    else if (t < hw + 24)
      o.sigs[k][16 * (uint64_t)d.slot + (t - hw - 8)] = rd_u32(w, f.idp + 32 + 4 * (t - hw - 8));
    else {
      const uint32_t v = (t - hw - 24) / 24, j = (t - hw - 24) % 24;
      uint64_t vp, L;
      if (r.vlen) {
        L = r.vlen;
        vp = f.vts + (uint64_t)v * (8 + L + 64);
      } else {
        for (; wv < v; ++wv) {
          if (wpos + 8 > off + len) return;
          const uint64_t l = rd_u64(w, wpos);
          if (l > len) return;
          wpos += 8 + l + 64;
        }
        if (wpos + 8 > off + len) return;
        vp = wpos;
        L = rd_u64(w, vp);
      }
      if (L > len || vp + 8 + L + 64 > off + len) return;
      const uint64_t vs = (uint64_t)d.vote0 + v;
      if (j < 8) o.vpk[8 * vs + j] = b64_word(w, vp + 8, j);
      else o.vsig[16 * vs + (j - 8)] = rd_u32(w, vp + 8 + L + 4 * (j - 8));
    }
  }
}

// Lane `lane` of `G` of the emit of one frame (r = its scan result, d = its destination): a
// Vote frame, or a Header / Certificate frame with a slot. Every write is checked against
// o's capacities, so a record and a destination that disagree write nothing out of bounds.
// kCanon = false: canonical frames only; c and order are never touched.
template <bool kCanon>
NW_HD void emit_lane(const uint32_t* w, uint64_t off, uint64_t len, const rec_t& r,
                     const canon_t* c, const uint32_t* order, uint64_t order_cap,
                     const dst_t& d, const out_t& o, uint32_t lane, uint32_t G) {
  if (d.slot == kNoSlot) return;
  if (r.kind == 1) {
    const vote_layout_t f = vote_layout(off, len, r);
    if (d.slot >= o.nvmsg || !f.ok) return;
    for (uint32_t t = lane; t < 42; t += G) {
      if (t < 8) o.v_ids[8 * (uint64_t)d.slot + t] = rd_u32(w, f.id + 4 * t);
      else if (t < 10)
        reinterpret_cast<uint32_t*>(o.v_rounds)[2 * (uint64_t)d.slot + (t - 8)] =
            rd_u32(w, f.rnd + 4 * (t - 8));
      else if (t < 18) o.v_origins[8 * (uint64_t)d.slot + (t - 10)] = b64_word(w, f.ot, t - 10);
      else if (t < 26) o.v_authors[8 * (uint64_t)d.slot + (t - 18)] = b64_word(w, f.at, t - 18);
      else o.v_sigs[16 * (uint64_t)d.slot + (t - 26)] = rd_u32(w, f.sg + 4 * (t - 26));
    }
    return;
  }
  if (r.kind != 0 && r.kind != 2) return;
  if (r.canonical) emit_header<false>(w, off, len, r, c, order, order_cap, d, o, lane, G);
  else if (kCanon) emit_header<true>(w, off, len, r, c, order, order_cap, d, o, lane, G);
}

}  // namespace wd
}  // namespace nw
