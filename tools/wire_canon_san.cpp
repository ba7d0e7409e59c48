// wire_canon_san.cpp — TEST INFRASTRUCTURE. A stand-alone host program that runs the device
// wire decoder's text (narwhal_amd/csrc/nw_wiredec.hpp, compiled as host code: scan,
// canon_stage / canon_mark / canon_rank, both instances of emit_lane) over generated frames
// and random mutations of them, with every buffer allocated at exactly the size the job
// gives it, so that AddressSanitizer / UBSan (`make wiresan`) see any read or write past a
// bound. CPU only; no device code runs.
//
//     tools/wire_canon_san [frames = 20000] [seed = 1]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "wire_single.hpp"

using namespace nw::wd;
typedef std::string bytes;

static std::mt19937_64 rng;
static uint64_t rnd(uint64_t n) { return n ? rng() % n : 0; }

static void put64(bytes& b, uint64_t v) { b.append(reinterpret_cast<const char*>(&v), 8); }
static void put32(bytes& b, uint32_t v) { b.append(reinterpret_cast<const char*>(&v), 4); }
static bytes rand_bytes(size_t n) {
  bytes b(n, 0);
  for (auto& c : b) c = (char)rng();
  return b;
}
static bytes b64(const bytes& in, bool pad) {
  static const char* T = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
  bytes o;
  size_t i = 0;
  for (; i + 3 <= in.size(); i += 3) {
    const uint32_t v = ((uint8_t)in[i] << 16) | ((uint8_t)in[i + 1] << 8) | (uint8_t)in[i + 2];
    o += T[v >> 18]; o += T[(v >> 12) & 63]; o += T[(v >> 6) & 63]; o += T[v & 63];
  }
  if (in.size() - i == 2) {
    const uint32_t v = ((uint8_t)in[i] << 16) | ((uint8_t)in[i + 1] << 8);
    o += T[v >> 18]; o += T[(v >> 12) & 63]; o += T[(v >> 6) & 63];
    if (pad) o += '=';
  } else if (in.size() - i == 1) {
    const uint32_t v = (uint8_t)in[i] << 16;
    o += T[v >> 18]; o += T[(v >> 12) & 63];
    if (pad) o += "==";
  }
  return o;
}
static void put_pk(bytes& b, const bytes& key, bool pad) {
  const bytes s = b64(key, pad);
  put64(b, s.size());
  b += s;
}

// One generated Header / Certificate and what BTreeMap / BTreeSet deserialisation makes of it.
struct gen_t {
  bytes frame, hb;       // hb = the `Hash for Header` bytes expected
  uint32_t np_u, nq_u;
  bool canonical;
};
static gen_t gen(uint32_t maxn) {
  gen_t g;
  const uint32_t variant = rnd(2) ? 2 : 0;
  const bytes author = rand_bytes(32), round = rand_bytes(8);
  // keys from a small pool (duplicates) that share long prefixes (the compare must go deep)
  std::vector<bytes> pool(1 + rnd(maxn));
  for (auto& k : pool) {
    k = bytes(32, (char)rnd(3));
    for (int t = 0, m = (int)rnd(4); t < m; ++t) k[rnd(32)] = (char)rng();
  }
  const uint32_t np = (uint32_t)rnd(maxn + 1), nq = (uint32_t)rnd(maxn + 1);
  std::vector<std::pair<bytes, uint32_t>> pay(np);
  std::vector<bytes> par(nq);
  for (auto& e : pay) e = {pool[rnd(pool.size())], (uint32_t)rng()};
  for (auto& e : par) e = pool[rnd(pool.size())];
  if (rnd(3) == 0) {   // often canonical as sent
    std::map<bytes, uint32_t> m(pay.begin(), pay.end());
    pay.assign(m.begin(), m.end());
    std::set<bytes> s(par.begin(), par.end());
    par.assign(s.begin(), s.end());
  }
  std::map<bytes, uint32_t> m;
  for (auto& e : pay) m[e.first] = e.second;   // the last value wins
  std::set<bytes> s(par.begin(), par.end());
  g.canonical = true;
  for (size_t i = 1; i < pay.size(); ++i) g.canonical &= pay[i - 1].first < pay[i].first;
  for (size_t i = 1; i < par.size(); ++i) g.canonical &= par[i - 1] < par[i];
  g.np_u = (uint32_t)m.size();
  g.nq_u = (uint32_t)s.size();
  g.hb = author + round;
  for (auto& e : m) {
    g.hb += e.first;
    put32(g.hb, e.second);
  }
  for (auto& e : s) g.hb += e;
  bytes& f = g.frame;
  put32(f, variant);
  put_pk(f, author, rnd(2));
  f += round;
  put64(f, pay.size());
  for (auto& e : pay) {
    f += e.first;
    put32(f, e.second);
  }
  put64(f, par.size());
  for (auto& e : par) f += e;
  f += rand_bytes(96);
  if (variant == 2) {
    const uint32_t nv = (uint32_t)rnd(5);
    put64(f, nv);
    const bool mixed = rnd(3) == 0;   // key texts of differing lengths: the emit walks
    for (uint32_t v = 0; v < nv; ++v) {
      put_pk(f, rand_bytes(32), mixed ? rnd(2) : true);
      f += rand_bytes(64);
    }
  }
  if (rnd(4) == 0) f += rand_bytes(rnd(9));   // trailing bytes are allowed
  return g;
}

static uint64_t g_done = 0, g_canon = 0, g_over = 0, g_bad = 0;

// The frame at byte offset mis of a word buffer that ends at the next multiple of 4 past the
// frame: what the decoder may read, and no more. expect: check the emitted rows against it.
static void run(const bytes& f, uint32_t mis, uint32_t lanes, uint32_t group, const gen_t* expect) {
  const uint64_t len = f.size();
  std::vector<uint32_t> w((mis + len + 3) / 4);
  if (w.empty()) w.resize(1);
  memset(w.data(), 0x5a, 4 * w.size());
  if (len) memcpy(reinterpret_cast<char*>(w.data()) + mis, f.data(), len);
  const rec_t r = scan(w.data(), mis, len);
  ++g_done;
  if (r.kind < 0) ++g_bad;
  if (expect && (r.kind != 0 && r.kind != 2)) abort();
  if (expect && (r.canonical != 0) != expect->canonical) abort();
  if (r.kind != 0 && r.kind != 2) {
    if (r.kind != 1) return;
    uint32_t ids[8], org[8], aut[8], sg[16];
    uint64_t round;
    wire_single_t s(1, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, ids, &round, org, aut,
                    sg);
    s.emit<false>(w.data(), mis, len, r, nullptr, nullptr, 0, group);
    return;
  }
  const wire_canon_t cr(w.data(), mis, len, r, lanes);
  const canon_t& c = cr.c;
  if (c.state == kCanonOver) ++g_over;
  if (c.state == kCanonDone) {
    ++g_canon;
    if (expect && (c.np_u != expect->np_u || c.nq_u != expect->nq_u)) abort();
  } else if (!r.canonical && c.state != kCanonOver) {
    abort();   // a record of this very frame always passes canon_begin's bounds
  }
  if (!r.canonical && c.state != kCanonDone) return;
  const uint64_t hl = r.canonical ? header_len(r.np, r.nq) : header_len(c.np_u, c.nq_u);
  std::vector<uint8_t> hb(hl);
  std::vector<uint32_t> id(8), sig(16), vpk(8 * (size_t)r.nv), vsig(16 * (size_t)r.nv);
  wire_single_t s(r.kind, hb.data(), hl, id.data(), sig.data(), vpk.data(), vsig.data(), r.nv,
                  nullptr, nullptr, nullptr, nullptr, nullptr);
  // a canonical frame: first the plain instance, which gets no canon_t and no order list
  if (r.canonical) s.emit<false>(w.data(), mis, len, r, nullptr, nullptr, 0, group);
  s.emit<true>(w.data(), mis, len, r, &c, cr.order.data(), cr.order.size(), group);
  if (expect) {
    // (the author's 32 bytes are the key's first 32; gen() encodes exactly 32)
    if (hl != expect->hb.size() || memcmp(hb.data(), expect->hb.data(), hl) != 0) abort();
    if (s.pc != expect->np_u) abort();
  }
}

int main(int argc, char** argv) {
  const long n = argc > 1 ? atol(argv[1]) : 20000;
  rng.seed(argc > 2 ? atoll(argv[2]) : 1);
  static const uint32_t kLanes[] = {1, 16, 64, 256}, kGroups[] = {1, 16, 64};
  for (long i = 0; i < n; ++i) {
    // mostly small frames; some at and over the entry bound
    const uint32_t maxn = i % 500 == 0 ? 700 : i % 50 == 0 ? 200 : 12;
    const gen_t g = gen(maxn);
    const uint32_t mis = (uint32_t)(i % 4), lanes = kLanes[(i / 4) % 4], group = kGroups[i % 3];
    run(g.frame, mis, lanes, group, &g);
    // mutations: a truncation, a flipped byte, a length prefix replaced
    bytes t = g.frame.substr(0, rnd(g.frame.size() + 1));
    run(t, mis, lanes, group, nullptr);
    bytes m = g.frame;
    for (int x = 0, e = 1 + (int)rnd(3); x < e; ++x) m[rnd(m.size())] ^= (char)(1 << rnd(8));
    run(m, mis, lanes, group, nullptr);
    if (m.size() > 80) {
      uint64_t v = rnd(4) == 0 ? rng() : rnd(2000);
      memcpy(&m[rnd(m.size() - 8)], &v, 8);
      run(m, mis, lanes, group, nullptr);
    }
  }
  printf("wire_canon_san: %llu frames run (%llu canonicalised, %llu over the bound, %llu undecodable): ok\n",
         (unsigned long long)g_done, (unsigned long long)g_canon, (unsigned long long)g_over,
         (unsigned long long)g_bad);
  return 0;
}
