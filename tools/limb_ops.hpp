// limb_ops.hpp — TEST INFRASTRUCTURE. One dispatcher over the per-lane field and point
// routines of nw_field.hpp / nw_point.hpp on RAW limbs, shared by tools/hostcheck.hip (the
// CPU build, hc_fe_ops / hc_ge_ops) and tools/lpcheck.hip (the gfx950 build, k_fe_ops), so
// that tests/test_field_limbs_cpu.py and tests/test_gpu_field_limbs.py run one set of
// operation codes (restated in tests/limb_cases.py) on both builds of the same text.
//
// A case is two operands of 40 words each, one integer and 40 words of output. A field
// element takes the first 10 words; a point is X, Y, Z, T (ge), a cached point YpX, YmX, Z2,
// T2d (ge_cached), an affine niels point ypx, ymx, xy2d (ge_niels) in that order.
#pragma once
#include "../narwhal_amd/csrc/nw_point.hpp"

namespace nw {

enum limb_op_code : int {
  // field: out = op(A[0..9], B[0..9], k)
  OP_FE_MUL = 0, OP_FE_SQ, OP_FE_SQN /* k squarings */, OP_FE_ADD, OP_FE_SUB, OP_FE_SUB_NC,
  OP_FE_NEG, OP_FE_NEG_NC, OP_FE_CARRY, OP_FE_CANONICAL,
  OP_FE_TOBYTES /* out: 8 words */, OP_FE_FROMBYTES /* A: 8 words */,
  OP_FE_ISZERO /* out[0] */, OP_FE_EQ /* out[0] */, OP_FE_ISNEGATIVE /* out[0] */,
  OP_FE_INVERT, OP_FE_POW22523,
  // points: out = X, Y, Z, T; k bit 0: want_t (T is left 0 without it), bit 1: affine
  OP_GE_DBL = 32, OP_GE_ADD_CACHED, OP_GE_SUB_CACHED, OP_GE_ADD_NIELS, OP_GE_ADD_ANY,
  OP_GE_ADD_ANY_NEGC,
};

NW_HD void limb_ld(fe& f, const uint32_t* w) {
#pragma unroll
  for (int i = 0; i < 10; ++i) f.v[i] = w[i];
}
NW_HD void limb_st(uint32_t* w, const fe& f) {
#pragma unroll
  for (int i = 0; i < 10; ++i) w[i] = f.v[i];
}

// false: unknown operation code (nothing written).
NW_HD bool limb_op(int op, const uint32_t* A, const uint32_t* B, int k, uint32_t* out) {
  if (op < OP_GE_DBL) {
    fe a, b, r;
    limb_ld(a, A);
    limb_ld(b, B);
    fe_0(r);
    switch (op) {
      case OP_FE_MUL: fe_mul(r, a, b); break;
      case OP_FE_SQ: fe_sq(r, a); break;
      case OP_FE_SQN: fe_sqn(r, a, k); break;
      case OP_FE_ADD: fe_add(r, a, b); break;
      case OP_FE_SUB: fe_sub(r, a, b); break;
      case OP_FE_SUB_NC: fe_sub_nc(r, a, b); break;
      case OP_FE_NEG: fe_neg(r, a); break;
      case OP_FE_NEG_NC: fe_neg_nc(r, a); break;
      case OP_FE_CARRY: fe_copy(r, a); fe_carry(r); break;
      case OP_FE_CANONICAL: fe_canonical(r, a); break;
      case OP_FE_TOBYTES: fe_tobytes(r.v, a); break;
      case OP_FE_FROMBYTES: fe_frombytes(r, A); break;
      case OP_FE_ISZERO: r.v[0] = fe_iszero(a) ? 1u : 0u; break;
      case OP_FE_EQ: r.v[0] = fe_eq(a, b) ? 1u : 0u; break;
      case OP_FE_ISNEGATIVE: r.v[0] = fe_isnegative(a); break;
      case OP_FE_INVERT: fe_invert(r, a); break;
      case OP_FE_POW22523: fe_pow22523(r, a); break;
      default: return false;
    }
    limb_st(out, r);
    return true;
  }
  ge p, r;
  ge_cached q;
  ge_niels n;
  limb_ld(p.X, A); limb_ld(p.Y, A + 10); limb_ld(p.Z, A + 20); limb_ld(p.T, A + 30);
  limb_ld(q.YpX, B); limb_ld(q.YmX, B + 10); limb_ld(q.Z2, B + 20); limb_ld(q.T2d, B + 30);
  limb_ld(n.ypx, B); limb_ld(n.ymx, B + 10); limb_ld(n.xy2d, B + 20);
  const bool want_t = (k & 1) != 0, affine = (k & 2) != 0;
  fe_0(r.T);
  switch (op) {
    case OP_GE_DBL: ge_dbl(r, p, want_t); break;
    case OP_GE_ADD_CACHED: ge_add_cached(r, p, q, want_t); break;
    case OP_GE_SUB_CACHED: ge_sub_cached(r, p, q, want_t); break;
    case OP_GE_ADD_NIELS: ge_add_niels(r, p, n, want_t); break;
    case OP_GE_ADD_ANY: ge_add_any(r, p, q, affine, want_t); break;
    case OP_GE_ADD_ANY_NEGC: ge_add_any_negc(r, p, q, affine, want_t); break;
    default: return false;
  }
  limb_st(out, r.X); limb_st(out + 10, r.Y); limb_st(out + 20, r.Z); limb_st(out + 30, r.T);
  return true;
}

}  // namespace nw
