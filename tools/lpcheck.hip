// lpcheck.hip — TEST INFRASTRUCTURE (tools/libnw_lpcheck.so; never linked into the product
// library). The per-lane field / point routines (nw_field.hpp, nw_point.hpp) and the limb-
// parallel routines (nw_lp.hpp) as gfx950 kernels over RAW limbs, for
// tests/test_gpu_field_limbs.py. Each entry takes host buffers, makes its own device copies,
// launches, synchronises and returns the HIP status (0 = hipSuccess; -1: bad argument).
//
//   k_fe_ops  one lane per case: tools/limb_ops.hpp's operation codes, as hc_fe_ops /
//             hc_ge_ops run them on the CPU build of the same text.
//   k_sc_ops  one lane per case: tools/sc_ops.hpp's operation codes over the scalar layer
//             (nw_scalar.hpp, the scalar phase of nw_strict.hpp), as hc_sc_ops runs them on
//             the CPU build, for tests/test_gpu_sc_ops.py.
//   k_lp_ops  one wave per case: operands are four planes of 64 words (plane p, lane l at
//             word 64 p + l; lane 16 r + k = limb k of row r), the output likewise.
// Both run at any block size that is a multiple of 64 with lane = tid & 63 (the product calls
// the limb-parallel code from 64-thread blocks, k_pip_final, and from 256-thread ones, k_small).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../narwhal_amd/csrc/nw_lp.hpp"
#include "limb_ops.hpp"
#include "sc_ops.hpp"

using namespace nw;

enum lp_op_code : int {
  LP_MUL = 0,           // out0 = lp_mul(in0, in1)
  LP_CARRY32,           // out0 = lp_carry32(in0)
  LP_SUB,               // out0 = lp_sub(in0, in1)
  LP_SUB_NC,            // out0 = lp_sub_nc(in0, in1)
  LP_ROWS_OF,           // out0..3 = lp_rows_of(in0).r0..r3
  LP_SEL,               // out0 = lp_sel(in0, in1, in2, in3)
  LP_IDENTITY,          // out0 = lp_identity()
  LP_DBL,               // out0 = lp_dbl(in0)
  LP_ADD,               // out0 = lp_add(in0, in1)
  LP_TO_CACHED,         // out0 = lp_to_cached(in0, d2l = in1)
  LP_CACHED_COMPONENT,  // out0 = lp_cached_component(ge_cached at in1[0..39])
  LP_NIELS_COMPONENT,   // out0 = lp_niels_component(ge_niels at in1[0..29], neg = k & 1)
  LP_IS_IDENTITY,       // out0 = lp_is_identity(in0) in every lane
  LP_SQN,               // out0 = lp_sqn(in0, k)
  LP_POW22523,          // out0 = lp_pow22523(in0)
  LP_CHAIN,             // out0 = lp_add(lp_dbl^k(in0), in1); out1 = per-lane maximum of every
                        // intermediate and the result (k_pip_final's Horner step)
  LP_N
};

constexpr int kLpWavesMax = 4;   // waves per block (block size <= 256)

__global__ __launch_bounds__(64 * kLpWavesMax) void k_fe_ops(
    int op, uint32_t n, const uint32_t* __restrict__ A, const uint32_t* __restrict__ B,
    const int32_t* __restrict__ k, uint32_t* __restrict__ out, uint32_t* __restrict__ bad) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (!limb_op(op, A + 40 * i, B + 40 * i, k[i], out + 40 * i)) *bad = 1u;
}

// One lane per case, lane = case index: the order of the cases decides which share a wave (the
// half-size split's one-step code runs only in an iteration where no lane of the wave made
// Lehmer progress, nw_scalar.hpp nw_any).
__global__ __launch_bounds__(64 * kLpWavesMax) void k_sc_ops(
    int op, uint32_t n, const uint32_t* __restrict__ in, const int32_t* __restrict__ k,
    uint32_t* __restrict__ out, uint32_t* __restrict__ bad) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (!sc_op(op, in + kScIn * i, k[i], out + kScOut * i)) *bad = 1u;
}

__global__ __launch_bounds__(64 * kLpWavesMax) void k_lp_ops(
    int op, uint32_t n, const uint32_t* __restrict__ in, const int32_t* __restrict__ kk,
    uint32_t* __restrict__ out) {
  __shared__ uint32_t s_tmp[kLpWavesMax][40];
  const uint32_t lane = threadIdx.x & 63u, wib = threadIdx.x >> 6;
  const uint64_t w = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (w >= n) return;   // wave-uniform
  const lp_ctx c = lp_init(lane);
  const uint32_t* I = in + 256 * w;
  uint32_t* O = out + 256 * w;
  const uint32_t a = I[lane], b = I[64 + lane];
  const int k = kk[w];
  uint32_t r = 0;
  switch (op) {   // uniform over the launch
    case LP_MUL: r = lp_mul(c, a, b); break;
    case LP_CARRY32: r = lp_carry32(c, a); break;
    case LP_SUB: r = lp_sub(c, a, b); break;
    case LP_SUB_NC: r = lp_sub_nc(c, a, b); break;
    case LP_ROWS_OF: {
      const lp_rows R = lp_rows_of(c, a);
      r = R.r0;
      O[64 + lane] = R.r1; O[128 + lane] = R.r2; O[192 + lane] = R.r3;
      break;
    }
    case LP_SEL: r = lp_sel(c, a, b, I[128 + lane], I[192 + lane]); break;
    case LP_IDENTITY: r = lp_identity(c); break;
    case LP_DBL: r = lp_dbl(c, a); break;
    case LP_ADD: r = lp_add(c, a, b); break;
    case LP_TO_CACHED: r = lp_to_cached(c, a, b); break;
    case LP_CACHED_COMPONENT:
      r = lp_cached_component(c, *reinterpret_cast<const ge_cached*>(I + 64));
      break;
    case LP_NIELS_COMPONENT:
      r = lp_niels_component(c, *reinterpret_cast<const ge_niels*>(I + 64), (k & 1) != 0);
      break;
    case LP_IS_IDENTITY: r = lp_is_identity(c, a, s_tmp[wib]) ? 1u : 0u; break;
    case LP_SQN: r = lp_sqn(c, a, k); break;
    case LP_POW22523: r = lp_pow22523(c, a); break;
    case LP_CHAIN: {
      uint32_t v = a, mx = 0;
#pragma unroll 1
      for (int i = 0; i < k; ++i) {
        v = lp_dbl(c, v);
        mx = v > mx ? v : mx;
      }
      v = lp_add(c, v, b);
      mx = v > mx ? v : mx;
      r = v;
      O[64 + lane] = mx;
      break;
    }
    default: break;
  }
  O[lane] = r;
}

namespace {

struct dev_buf {
  void* p = nullptr;
  ~dev_buf() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 4); }
  template <class T> T* as() const { return static_cast<T*>(p); }
};

#define LPC_TRY(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

bool block_ok(int block) { return block >= 64 && block <= 64 * kLpWavesMax && block % 64 == 0; }

}  // namespace

extern "C" {

// n cases of one limb_ops.hpp operation, one lane each: A, B n x 40 words, k n integers,
// out n x 40 words.
int lpc_fe_ops(int op, uint32_t n, const uint32_t* A, const uint32_t* B, const int32_t* k,
               uint32_t* out, int block) {
  if (!block_ok(block) || n == 0 || n > (1u << 24)) return -1;
  const size_t words = 40 * (size_t)n;
  dev_buf dA, dB, dk, dout, dbad;
  LPC_TRY(dA.alloc(4 * words)); LPC_TRY(dB.alloc(4 * words)); LPC_TRY(dk.alloc(4 * (size_t)n));
  LPC_TRY(dout.alloc(4 * words)); LPC_TRY(dbad.alloc(4));
  LPC_TRY(hipMemcpy(dA.p, A, 4 * words, hipMemcpyHostToDevice));
  LPC_TRY(hipMemcpy(dB.p, B, 4 * words, hipMemcpyHostToDevice));
  LPC_TRY(hipMemcpy(dk.p, k, 4 * (size_t)n, hipMemcpyHostToDevice));
  LPC_TRY(hipMemset(dout.p, 0, 4 * words));
  LPC_TRY(hipMemset(dbad.p, 0, 4));
  const uint32_t grid = (uint32_t)(((uint64_t)n + block - 1) / block);
  hipLaunchKernelGGL(k_fe_ops, dim3(grid), dim3(block), 0, 0, op, n, dA.as<uint32_t>(),
                     dB.as<uint32_t>(), dk.as<int32_t>(), dout.as<uint32_t>(), dbad.as<uint32_t>());
  LPC_TRY(hipGetLastError());
  LPC_TRY(hipDeviceSynchronize());
  uint32_t bad = 0;
  LPC_TRY(hipMemcpy(&bad, dbad.p, 4, hipMemcpyDeviceToHost));
  LPC_TRY(hipMemcpy(out, dout.p, 4 * words, hipMemcpyDeviceToHost));
  return bad ? -1 : 0;
}

// n cases of one sc_ops.hpp operation, one lane each (lane = case index & 63): in n x 24 words,
// k n integers, out n x 40 words.
int lpc_sc_ops(int op, uint32_t n, const uint32_t* in, const int32_t* k, uint32_t* out, int block) {
  if (!block_ok(block) || n == 0 || n > (1u << 24) || op < 0 || op >= SC_N) return -1;
  const size_t wi = kScIn * (size_t)n, wo = kScOut * (size_t)n;
  dev_buf din, dk, dout, dbad;
  LPC_TRY(din.alloc(4 * wi)); LPC_TRY(dk.alloc(4 * (size_t)n));
  LPC_TRY(dout.alloc(4 * wo)); LPC_TRY(dbad.alloc(4));
  LPC_TRY(hipMemcpy(din.p, in, 4 * wi, hipMemcpyHostToDevice));
  LPC_TRY(hipMemcpy(dk.p, k, 4 * (size_t)n, hipMemcpyHostToDevice));
  LPC_TRY(hipMemset(dout.p, 0, 4 * wo));
  LPC_TRY(hipMemset(dbad.p, 0, 4));
  const uint32_t grid = (uint32_t)(((uint64_t)n + block - 1) / block);
  hipLaunchKernelGGL(k_sc_ops, dim3(grid), dim3(block), 0, 0, op, n, din.as<uint32_t>(),
                     dk.as<int32_t>(), dout.as<uint32_t>(), dbad.as<uint32_t>());
  LPC_TRY(hipGetLastError());
  LPC_TRY(hipDeviceSynchronize());
  uint32_t bad = 0;
  LPC_TRY(hipMemcpy(&bad, dbad.p, 4, hipMemcpyDeviceToHost));
  LPC_TRY(hipMemcpy(out, dout.p, 4 * wo, hipMemcpyDeviceToHost));
  return bad ? -1 : 0;
}

// n cases of one limb-parallel operation, one wave each: in n x 256 words (four planes),
// k n integers, out n x 256 words.
int lpc_lp_ops(int op, uint32_t n, const uint32_t* in, const int32_t* k, uint32_t* out,
               int block) {
  if (!block_ok(block) || n == 0 || n > (1u << 20) || op < 0 || op >= LP_N) return -1;
  const size_t words = 256 * (size_t)n;
  dev_buf din, dk, dout;
  LPC_TRY(din.alloc(4 * words)); LPC_TRY(dk.alloc(4 * (size_t)n)); LPC_TRY(dout.alloc(4 * words));
  LPC_TRY(hipMemcpy(din.p, in, 4 * words, hipMemcpyHostToDevice));
  LPC_TRY(hipMemcpy(dk.p, k, 4 * (size_t)n, hipMemcpyHostToDevice));
  LPC_TRY(hipMemset(dout.p, 0, 4 * words));
  const uint32_t per = (uint32_t)block / 64u;
  const uint32_t grid = (n + per - 1) / per;
  hipLaunchKernelGGL(k_lp_ops, dim3(grid), dim3(block), 0, 0, op, n, din.as<uint32_t>(),
                     dk.as<int32_t>(), dout.as<uint32_t>());
  LPC_TRY(hipGetLastError());
  LPC_TRY(hipDeviceSynchronize());
  LPC_TRY(hipMemcpy(out, dout.p, 4 * words, hipMemcpyDeviceToHost));
  return 0;
}

}
