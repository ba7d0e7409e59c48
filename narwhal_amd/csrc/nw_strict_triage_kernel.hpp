// nw_strict_triage_kernel.hpp — the text of the two-pass launch's triage kernel (nw_kernels.hip
// "config 4's strict verification in two passes"), included there once per instance with
//   NW_TRIAGE_KERNEL  the kernel's name
//   NW_TRIAGE_SRC     the source of an item's inputs: strict_src_global (k_strict_triage: k is
//                     hashed from 32 message bytes) or strict_src_plane (k_strict_triage_k: msgs
//                     is the k plane of a launch over messages of any length)
// defined. The instances are kernels in their own right, not a shared inlined body: as a body
// inlined into two kernels the compiler scheduled k_strict_triage differently, and that
// kernel's code object is to stay what it was. No include guard.
#if !defined(NW_TRIAGE_KERNEL) || !defined(NW_TRIAGE_SRC)
#error "define NW_TRIAGE_KERNEL and NW_TRIAGE_SRC before including nw_strict_triage_kernel.hpp"
#endif
__global__ __launch_bounds__(256, NW_TRIAGE_WAVES) void NW_TRIAGE_KERNEL(
    const uint32_t* __restrict__ msgs, uint32_t msg_stride_words, const uint32_t* __restrict__ pks,
    const uint32_t* __restrict__ sigs, uint64_t i0, uint64_t ns, int32_t* __restrict__ status,
    uint32_t* __restrict__ xs, uint64_t cap, uint32_t* __restrict__ list,
    uint32_t* __restrict__ count, const uint32_t* __restrict__ keyslot,
    const uint32_t* __restrict__ kflags, const uint32_t* __restrict__ todo,
    const uint32_t* __restrict__ todo_count, unsigned long long* __restrict__ todo_total,
    const uint32_t* __restrict__ nhot, unsigned long long* __restrict__ settled) {
  // todo == nullptr, or no hot key in the slice (*nhot == 0: the comb kernels did nothing):
  // lane q takes item q of the slice; else the item of entry todo[q], q < *todo_count (the items
  // the comb check did not pass, k_strict_todo_list). An entry with kTodoDecided set is an item
  // whose comb sum ran and gave R' != decode(R): its status is the triage's own if the triage
  // rejects it (R does not decode), else NW_ERR_EQUATION (comb_settled_status); either way it is
  // settled here and never reaches the ladder. settled[wave & (kCombStatLanes - 1)] += the
  // wave's items settled as equation failures (diagnostics, one atomic per wave that has any).
  const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (todo && *nhot == 0) todo = nullptr;
  const uint64_t nq = todo ? (uint64_t)*todo_count : ns;
  const bool active = q < nq;
  // *todo_total += the slice's items that come here (diagnostics, kept over a launch's slices)
  if (todo_total && q == 0) atomicAdd(todo_total, (unsigned long long)nq);
  if (__ballot(active) == 0) return;
  const uint32_t entry = todo ? todo[active ? q : 0] : (uint32_t)q;
  const bool decided = todo && (entry & kTodoDecided) != 0;
  const uint64_t j = todo ? (uint64_t)comb_todo_item(entry) : q;
  const uint64_t i = i0 + (active ? j : 0);
  const NW_TRIAGE_SRC src{pks + 8 * i, sigs + 16 * i, msgs + (uint64_t)msg_stride_words * i};
  // the key's slot in the slice's set (keyslot == nullptr: the set is off); an idle lane of the
  // last wave takes item i0's
  const uint32_t slot = keyslot ? keyslot[active ? j : 0] : kNoSlot;
  const uint32_t keyflags = slot != kNoSlot ? kflags[slot] : kNoSlot;
  fe xa, xr;
  const int st = strict_triage(src, g_consts.sk, xa, xr, keyflags,
                               [](bool b) { return __ballot(b) != 0; });
  // (comb_settled_status of a rejected item is the triage's status, decided or not)
  if (active && (st != NW_OK || decided)) status[i] = comb_settled_status(st);
  const uint32_t lane = threadIdx.x & 63u;
  if (todo) {
    const uint64_t ms = __ballot(active && decided && st == NW_OK);
    if (ms && lane == (uint32_t)__builtin_ctzll(ms))
      atomicAdd(settled + ((q >> 6) & (kCombStatLanes - 1)),
                (unsigned long long)__builtin_popcountll(ms));
  }
  const bool keep = active && st == NW_OK && !decided;
  const uint64_t m = __ballot(keep);
  if (m == 0) return;
  const uint32_t rank = (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
  const uint32_t leader = (uint32_t)__builtin_ctzll(m);
  uint32_t base = 0;
  if (lane == leader) base = atomicAdd(count, (uint32_t)__builtin_popcountll(m));
  base = (uint32_t)__shfl((int)base, (int)leader);
  if (!keep) return;
  const uint64_t pos = (uint64_t)base + rank;
  list[pos] = (uint32_t)j;
  if (slot != kNoSlot) {
    xs[pos] = slot;
  } else {
#pragma unroll
    for (int k = 0; k < 10; ++k) xs[(uint64_t)k * cap + pos] = xa.v[k];
  }
#pragma unroll
  for (int k = 0; k < 10; ++k) xs[(uint64_t)(10 + k) * cap + pos] = xr.v[k];
  // the survivors' scalar phase, after the x limbs are stored (nothing of the decompression
  // is live here); the lanes of rejected items have left
  uint32_t dig[kStrictDigitWords], meta;
  strict_triage_scalars<NW_BWIN>(src, dig, meta);
#pragma unroll
  for (int t = 0; t < kStrictDigitWords; ++t) xs[(uint64_t)(20 + t) * cap + pos] = dig[t];
  xs[(uint64_t)(20 + kStrictDigitWords) * cap + pos] = meta | (slot != kNoSlot ? kMetaSharedA : 0u);
}
#undef NW_TRIAGE_KERNEL
#undef NW_TRIAGE_SRC
