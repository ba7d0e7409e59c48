// stagecheck.hip — TEST INFRASTRUCTURE. Runs the message jobs' staging layout
// (narwhal_amd/csrc/nw_stage.hpp: plan, fill, view) over plain malloc'ed buffers through a C
// ABI, so tests/test_stage_cpu.py can pin every section offset and read every staged array
// back without a GPU. As the jobs do, the groups are planned behind the committee and the
// status and index sections behind the groups; the inputs are filled into one buffer, copied
// to a second one (as NW_SMALL_VRAM copies [0, o_st)) and viewed through that copy. Both
// buffers have exactly the planned size, so the stand-alone form (`make stagesan`, this file
// with its main under AddressSanitizer / UBSan) sees any access past a section's end.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../narwhal_amd/csrc/nw_stage.hpp"

namespace stg = nw::stage;

enum { kHeaders = 0, kCerts = 1, kVotes = 2 };
enum { kSections = 18 };   // committee 4, header stream 5, certificate votes 4, Vote messages 5

struct sc_staged {
  char* copy;                        // the inputs, [0, o_st), where the views look
  const void* view[kSections];       // null: not staged
  size_t bytes[kSections];
};

extern "C" {

// offs: kSections section offsets in the order above (UINT64_MAX: not staged), then o_st, o_ix
// and the buffer's end. z16 / with_vo: certificates only.
sc_staged* sc_stage(const nw_committee* com, int kind, const nw_certificates* cs,
                    const uint8_t* z16, int with_vo, const stg::VoteMsgs* va, uint64_t* offs) {
  const size_t n = kind == kVotes ? va->n : cs->n;
  const size_t nv = kind == kCerts ? cs->vote_offsets[n] : 0;
  stg::Packer P;
  const stg::CommitteeOffs oc = stg::plan_committee(P, com);
  stg::HeaderOffs oh;
  stg::CertVoteOffs ov;
  stg::VoteMsgOffs om;
  size_t hlen = 0;
  if (kind == kVotes) {
    om = stg::plan_vote_msgs(P, n);
  } else {
    hlen = cs->header_offsets[n] - cs->header_offsets[0];
    oh = stg::plan_headers(P, n, hlen);
    if (kind == kCerts) ov = stg::plan_cert_votes(P, n, nv, with_vo != 0, z16 != nullptr);
  }
  const size_t o_st = P.add(4 * n), o_ix = P.add(8 * n);
  char* h = static_cast<char*>(malloc(P.off));
  memset(h, 0xEE, P.off);
  stg::fill_committee(h, oc, com);
  if (kind == kVotes) {
    stg::fill_vote_msgs(h, om, *va);
  } else {
    stg::fill_headers(h, oh, cs);
    if (kind == kCerts) stg::fill_cert_votes(h, ov, cs, z16);
  }
  sc_staged* s = new sc_staged;
  s->copy = static_cast<char*>(malloc(o_st));
  memcpy(s->copy, h, o_st);
  free(h);
  const nw_committee c = stg::view_committee(s->copy, oc, com->nauth);
  nw_certificates d = stg::view_headers(s->copy, oh, n, hlen);
  const uint8_t* dz = stg::view_cert_votes(s->copy, ov, nv, &d);
  const stg::VoteMsgs v = stg::view_vote_msgs(s->copy, om, n);
  const stg::Sec secs[kSections] = {oc.pks, oc.stakes, oc.wo, oc.wi, oh.hb, oh.ho,
                                    oh.pc,  oh.id,     oh.hs, ov.vo, ov.vp, ov.vs,
                                    ov.z,   om.id,     om.rd, om.org, om.au, om.sg};
  const void* views[kSections] = {c.pks, c.stakes, c.worker_offsets, c.worker_ids,
                                  d.header_bytes, d.header_offsets, d.payload_counts, d.ids,
                                  d.header_sigs, d.vote_offsets, d.vote_pks, d.vote_sigs, dz,
                                  v.ids, v.rounds, v.origins, v.authors, v.sigs};
  for (int i = 0; i < kSections; ++i) {
    offs[i] = secs[i].staged() ? secs[i].off : ~0ull;
    s->view[i] = views[i];
    s->bytes[i] = secs[i].bytes;
  }
  offs[kSections] = o_st;
  offs[kSections + 1] = o_ix;
  offs[kSections + 2] = P.off;
  return s;
}

// Section `which` as its view reads it: copies its bytes to dst and returns their count, or
// -1 when the view is null (not staged).
long sc_read(const sc_staged* s, int which, void* dst) {
  if (!s->view[which]) return -1;
  if (s->bytes[which]) memcpy(dst, s->view[which], s->bytes[which]);
  return (long)s->bytes[which];
}

void sc_free(sc_staged* s) {
  free(s->copy);
  delete s;
}

}  // extern "C"

#ifdef STAGECHECK_MAIN
// The cases of tests/test_stage_cpu.py over generated arrays of the same shapes (the staging
// never looks into the bytes), every source array allocated at exactly its size.
static std::vector<uint8_t> fill(size_t bytes, uint8_t seed) {
  std::vector<uint8_t> v(bytes);
  for (size_t i = 0; i < bytes; ++i) v[i] = (uint8_t)(seed + 31 * i);
  return v;
}
static int g_bad = 0;
static void expect_read(const sc_staged* s, int which, const void* src, size_t bytes) {
  std::vector<uint8_t> got(bytes + 1);
  if (sc_read(s, which, got.data()) != (long)bytes || (bytes && memcmp(got.data(), src, bytes))) {
    fprintf(stderr, "section %d does not read back\n", which);
    ++g_bad;
  }
}

static void run(size_t na, size_t nwk, size_t n, size_t a, size_t votes_each) {
  // committee (the last authority owns every worker id)
  const std::vector<uint8_t> pks = fill(32 * na, 1), ids = fill(32 * n, 2), hs = fill(64 * n, 3);
  std::vector<uint32_t> stakes(na, 1), wi(nwk, 7), pc(n, 2);
  std::vector<uint64_t> wo(na + 1, 0), ho(n + 1), vo(n + 1);
  wo[na] = nwk;
  for (size_t i = 0; i <= n; ++i) {
    ho[i] = 40 * i + 36 * (i * (i + 1) / 2);   // headers of growing length
    vo[i] = votes_each * i;
  }
  const size_t nv = vo[n];
  const std::vector<uint8_t> hb = fill(ho[n], 4), vp = fill(32 * nv, 5), vs = fill(64 * nv, 6),
                             z = fill(16 * nv, 7), org = fill(32 * n, 8), au = fill(32 * n, 9);
  const std::vector<uint64_t> rounds(n, 11);
  const nw_committee com{na, pks.data(), stakes.data(), wo.data(), wi.data()};
  // messages [a, n), as a fan-out part: absolute header offsets, rebased vote offsets
  const size_t m = n - a;
  std::vector<uint64_t> pvo(m + 1);
  for (size_t i = 0; i <= m; ++i) pvo[i] = vo[a + i] - vo[a];
  nw_certificates cs{};
  cs.n = m;
  cs.header_bytes = hb.data();
  cs.header_offsets = ho.data() + a;
  cs.payload_counts = pc.data() + a;
  cs.ids = ids.data() + 32 * a;
  cs.header_sigs = hs.data() + 64 * a;
  cs.vote_offsets = pvo.data();
  cs.vote_pks = vp.data() + 32 * vo[a];
  cs.vote_sigs = vs.data() + 64 * vo[a];
  const size_t pnv = pvo[m];
  const stg::VoteMsgs va{ids.data() + 32 * a, rounds.data() + a, org.data() + 32 * a,
                         au.data() + 32 * a, hs.data() + 64 * a, m};
  uint64_t offs[kSections + 3];
  for (int kind = kHeaders; kind <= kVotes; ++kind)
    for (int opt = 0; opt < (kind == kCerts ? 4 : 1); ++opt) {
      const uint8_t* pz = (opt & 1) ? z.data() + 16 * vo[a] : nullptr;
      sc_staged* s = sc_stage(&com, kind, &cs, pz, opt & 2, &va, offs);
      expect_read(s, 0, pks.data(), 32 * na);
      expect_read(s, 1, stakes.data(), 4 * na);
      expect_read(s, 2, wo.data(), 8 * (na + 1));
      expect_read(s, 3, wi.data(), 4 * nwk);
      if (kind == kVotes) {
        expect_read(s, 13, va.ids, 32 * m);
        expect_read(s, 14, va.rounds, 8 * m);
        expect_read(s, 15, va.origins, 32 * m);
        expect_read(s, 16, va.authors, 32 * m);
        expect_read(s, 17, va.sigs, 64 * m);
      } else {
        std::vector<uint64_t> rho(m + 1);
        for (size_t i = 0; i <= m; ++i) rho[i] = ho[a + i] - ho[a];
        expect_read(s, 4, hb.data() + ho[a], ho[n] - ho[a]);
        expect_read(s, 5, rho.data(), 8 * (m + 1));
        expect_read(s, 6, cs.payload_counts, 4 * m);
        expect_read(s, 7, cs.ids, 32 * m);
        expect_read(s, 8, cs.header_sigs, 64 * m);
        if (kind == kCerts) {
          if (opt & 2) expect_read(s, 9, pvo.data(), 8 * (m + 1));
          expect_read(s, 10, cs.vote_pks, 32 * pnv);
          expect_read(s, 11, cs.vote_sigs, 64 * pnv);
          if (pz) expect_read(s, 12, pz, 16 * pnv);
        }
      }
      sc_free(s);
    }
}

int main() {
  run(4, 4, 14, 0, 3);
  run(4, 4, 14, 5, 3);   // a slice: header_offsets[0] != 0
  run(4, 0, 14, 0, 3);   // no worker ids
  run(4, 4, 14, 0, 0);   // no votes
  run(1, 1, 1, 0, 1);
  if (g_bad) return 1;
  printf("stagecheck ok\n");
  return 0;
}
#endif
