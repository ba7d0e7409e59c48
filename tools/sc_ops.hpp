// sc_ops.hpp — TEST INFRASTRUCTURE. One dispatcher over the scalar layer (nw_scalar.hpp: Barrett
// reduction, sc_mul / sc_add / sc_neg / sc_is_canonical, sc_recode, the half-size split) and the
// scalar phase of nw_strict.hpp (strict_scalar_phase, bdigits, key_recode / key_digit) on RAW
// words, shared by tools/hostcheck.hip (the CPU build, hc_sc_ops) and tools/lpcheck.hip (the
// gfx950 build, k_sc_ops), so that tests/test_sc_ops_cpu.py and tests/test_gpu_sc_ops.py run
// one set of operation codes (restated in tests/sc_cases.py) on both builds of the same text.
//
// A case is kScIn = 24 words of input, one integer and kScOut = 40 words of output; words an
// operation does not write stay as the caller left them (the entries zero them).
#pragma once
#include "../narwhal_amd/csrc/nw_strict.hpp"

namespace nw {

enum sc_op_code : int {
  SC_REDUCE512 = 0,        // in[0..15] -> out[0..7]
  SC_MUL,                  // in[0..7] * in[8..15] -> out[0..7]
  SC_ADD,                  // in[0..7] + in[8..15] -> out[0..7]
  SC_NEG,                  // -in[0..7] -> out[0..7]
  SC_CANONICAL,            // out[0] = sc_is_canonical(in[0..7])
  SC_RECODE,               // out[0..7] = sc_recode(in[0..7], bias word (uint32_t)k)
  SC_HALF_SPLIT,           // sc_half_split<true>(in[0..7]): out = u[8], v[5], vneg
  SC_HALF_SPLIT_ONESTEP,   // sc_half_split<false>, the same layout
  SC_SCALAR_PHASE_16,      // strict_scalar_phase<16>(k = in[0..7], s = in[8..15]):
  SC_SCALAR_PHASE_24,      //   out = dig[21], vneg, W
  SC_BDIGITS_8,            // bdigits<BW>::recode(in[0..7]) -> out[0..7], then digit(out, m),
  SC_BDIGITS_16,           //   m < NB, as int32 at out[8 + m]
  SC_BDIGITS_20,
  SC_BDIGITS_24,
  SC_KEY_DIGITS,           // key_recode / key_digit under keyspec_for(k), k in {8, 16, 20, 24}:
                           //   out[0..7], then digit t < ntab at out[8 + t]
  SC_N
};

constexpr int kScIn = 24, kScOut = 40;

NW_HD void sc_ld(sc& s, const uint32_t* w) {
#pragma unroll
  for (int i = 0; i < 8; ++i) s.w[i] = w[i];
}
NW_HD void sc_st(uint32_t* w, const sc& s) {
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = s.w[i];
}

template <bool LEHMER>
NW_HD void sc_op_half(const sc& k, uint32_t* out) {
  sc_half h;
  sc_half_split<LEHMER>(h, k);
#pragma unroll
  for (int i = 0; i < 8; ++i) out[i] = h.u[i];
#pragma unroll
  for (int i = 0; i < 5; ++i) out[8 + i] = h.v[i];
  out[13] = h.vneg ? 1u : 0u;
}

template <int BW>
NW_HD void sc_op_phase(const sc& k, const sc& s, uint32_t* out) {
  uint32_t dig[kStrictDigitWords];
  bool vneg;
  int W;
  strict_scalar_phase<BW>(dig, vneg, W, k, s);
#pragma unroll
  for (int i = 0; i < kStrictDigitWords; ++i) out[i] = dig[i];
  out[kStrictDigitWords] = vneg ? 1u : 0u;
  out[kStrictDigitWords + 1] = (uint32_t)W;
}

template <int BW>
NW_HD void sc_op_bdigits(const sc& w, uint32_t* out) {
  uint32_t wd[8];
  bdigits<BW>::recode(wd, w);
#pragma unroll
  for (int i = 0; i < 8; ++i) out[i] = wd[i];
#pragma unroll 1
  for (int m = 0; m < bdigits<BW>::NB; ++m) out[8 + m] = (uint32_t)bdigits<BW>::digit(wd, m);
}

// false: unknown operation code, or a key width keyspec_for does not build (nothing written).
NW_HD bool sc_op(int op, const uint32_t* in, int k, uint32_t* out) {
  sc a, b, r;
  sc_ld(a, in);
  sc_ld(b, in + 8);
  switch (op) {
    case SC_REDUCE512: sc_reduce512(r, in); sc_st(out, r); break;
    case SC_MUL: sc_mul(r, a, b); sc_st(out, r); break;
    case SC_ADD: sc_add(r, a, b); sc_st(out, r); break;
    case SC_NEG: sc_neg(r, a); sc_st(out, r); break;
    case SC_CANONICAL: out[0] = sc_is_canonical(a) ? 1u : 0u; break;
    case SC_RECODE: sc_recode(out, a, (uint32_t)k); break;
    case SC_HALF_SPLIT: sc_op_half<true>(a, out); break;
    case SC_HALF_SPLIT_ONESTEP: sc_op_half<false>(a, out); break;
    case SC_SCALAR_PHASE_16: sc_op_phase<16>(a, b, out); break;
    case SC_SCALAR_PHASE_24: sc_op_phase<24>(a, b, out); break;
    case SC_BDIGITS_8: sc_op_bdigits<8>(a, out); break;
    case SC_BDIGITS_16: sc_op_bdigits<16>(a, out); break;
    case SC_BDIGITS_20: sc_op_bdigits<20>(a, out); break;
    case SC_BDIGITS_24: sc_op_bdigits<24>(a, out); break;
    case SC_KEY_DIGITS: {
      const keyspec ks = keyspec_for((uint32_t)k);
      if (ks.W != (uint32_t)k) return false;
      uint32_t kd[8];
      key_recode(kd, a, ks);
#pragma unroll
      for (int i = 0; i < 8; ++i) out[i] = kd[i];
#pragma unroll 1
      for (uint32_t t = 0; t < ks.ntab; ++t) out[8 + t] = (uint32_t)key_digit(kd, (int)t, ks);
      break;
    }
    default: return false;
  }
  return true;
}

}  // namespace nw
