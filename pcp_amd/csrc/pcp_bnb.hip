// pcp_bnb.hip — branch and bound around the propagation fixpoint (gfx950, wave64): the two small kernels of pcp_propagate_device_bnb.
//
// The reference's BranchAndBound (search/branch_and_bound.rs:64-84) gives every node it enters, once a solution is known, one more unary
// propagator: XLessY(var, Constant(best)) when minimising, x_greater_y(var, Constant(best)) when maximising.  Such a propagator narrows its
// variable on its first run and is then entailed (x_less_y.rs:87-109), so it is FOLDED into the node's domain before the fixpoint, exactly
// as BinarySplit's branch constraints are (pcp_branch_device).  When the node comes out Satisfiable the incumbent becomes var.lower() — in
// both modes.  Batched, the rule becomes: fold every node of the batch against the incumbent as it stands on the device, run the fixpoint,
// then let the best Satisfiable node of the batch (ties: lowest index) replace the incumbent if it beats it.
//
//   bnb_fold_kernel   one lane per node, before the fixpoint: reads the incumbent and the objective's column (interval mode: one bound;
//                     set mode: the objective's set_words words) and narrows it.  A node the fold would EMPTY is left as it is — a valid
//                     row, so no kernel path's hull check or sticky flag sees it — and marked in the context's scratch.
//   bnb_reduce_kernel one workgroup, after the fixpoint: forces the marked nodes to PCP_FALSE (a node the fixpoint refused keeps
//                     PCP_STATUS_HULL), takes the best lb_out[var] of the PCP_TRUE nodes as a (key, index) minimum, and when it beats the
//                     incumbent writes the incumbent, copies the winning row(s) and bumps `improved`.
// Both are a few microseconds at any batch size the drivers use; the fixpoint between them is untouched (fusing the fold into each kernel
// family's staging is left for later; smallexcl_kernel<true>, pcp_smallexcl.hip, does fold while it stages and leaves the marks for the reduce).
// Vector memory operations only.
#include "pcp_internal.h"

namespace pcp {

namespace {

constexpr uint32_t kFoldThreads = 256;
constexpr uint32_t kReduceThreads = 1024;  // 16 wavefronts

// Word w of the mask that keeps bit indices first..last of a set (bit 64 w + b = value base + 64 w + b).
__device__ __forceinline__ uint64_t keep_mask(int64_t first, int64_t last, uint32_t w) {
  const int64_t lo = 64 * (int64_t)w, hi = lo + 63;
  if (last < lo || first > hi || first > last) return 0ull;
  uint64_t m = ~0ull;
  if (first > lo) m &= ~0ull << (uint32_t)(first - lo);
  if (last < hi) m &= ~0ull >> (uint32_t)(hi - last);
  return m;
}

__global__ void __launch_bounds__(kFoldThreads) bnb_fold_kernel(uint32_t n_nodes, uint32_t n_vars, uint32_t var, uint32_t mode, const int32_t* __restrict__ best,
                                                                int32_t* __restrict__ lb, int32_t* __restrict__ ub, uint64_t* __restrict__ bits,
                                                                uint32_t set_words, int32_t base, uint8_t* __restrict__ empty) {
  const uint32_t i = blockIdx.x * kFoldThreads + threadIdx.x;
  if (i >= n_nodes) return;
  const int64_t b = *best;
  uint8_t e = 0;
  if (bits) {
    // values <= best - 1 (minimize) or >= best + 1 (maximize) stay, as bit indices (v - base); int64: "none" is +-(2^29) and base any int32
    const int64_t first = mode == PCP_MINIMIZE ? INT64_MIN / 2 : b + 1 - base;
    const int64_t last = mode == PCP_MINIMIZE ? b - 1 - base : INT64_MAX / 2;
    uint64_t* row = bits + ((size_t)i * n_vars + var) * set_words;
    uint64_t any = 0;
    for (uint32_t w = 0; w < set_words; ++w) any |= row[w] & keep_mask(first, last, w);
    if (any) {
      for (uint32_t w = 0; w < set_words; ++w) {
        const uint64_t old = row[w], now = old & keep_mask(first, last, w);
        if (now != old) row[w] = now;
      }
    } else {
      e = 1;
    }
  } else {
    const size_t o = (size_t)i * n_vars + var;
    const int64_t l = lb[o], u = ub[o];
    if (mode == PCP_MINIMIZE) {
      if (b - 1 < u) {
        if (b - 1 < l) e = 1;
        else ub[o] = (int32_t)(b - 1);
      }
    } else if (b + 1 > l) {
      if (b + 1 > u) e = 1;
      else lb[o] = (int32_t)(b + 1);
    }
  }
  empty[i] = e;
}

// Order key of a candidate: smaller is better, the node index breaks ties (lowest wins).
__device__ __forceinline__ unsigned long long cand_key(int32_t v, uint32_t mode, uint32_t i) {
  const uint32_t biased = (uint32_t)v ^ 0x80000000u;  // signed order as unsigned order
  return ((unsigned long long)(mode == PCP_MINIMIZE ? biased : ~biased) << 32) | i;
}

__global__ void __launch_bounds__(kReduceThreads) bnb_reduce_kernel(uint32_t n_nodes, uint32_t n_vars, uint32_t var, uint32_t mode, const uint8_t* __restrict__ empty,
                                                                    uint8_t* __restrict__ status, const int32_t* __restrict__ lb_out,
                                                                    const int32_t* __restrict__ ub_out, const uint64_t* __restrict__ bits_out,
                                                                    uint32_t set_words, int32_t* __restrict__ best, int32_t* __restrict__ best_lb,
                                                                    int32_t* __restrict__ best_ub, uint64_t* __restrict__ best_bits,
                                                                    uint32_t* __restrict__ improved) {
  __shared__ unsigned long long wave_min[kReduceThreads / 64];
  __shared__ int32_t winner;
  unsigned long long k = ~0ull;
  for (uint32_t i = threadIdx.x; i < n_nodes; i += kReduceThreads) {
    const uint8_t s = status[i];
    if (empty[i]) {
      if (s != PCP_STATUS_HULL && s != PCP_FALSE) status[i] = PCP_FALSE;
      continue;
    }
    if (s == PCP_TRUE) {
      const unsigned long long c = cand_key(lb_out[(size_t)i * n_vars + var], mode, i);
      k = c < k ? c : k;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(k, off, 64);
    k = o < k ? o : k;
  }
  if ((threadIdx.x & 63) == 0) wave_min[threadIdx.x >> 6] = k;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long m = ~0ull;
    for (uint32_t w = 0; w < kReduceThreads / 64; ++w) m = wave_min[w] < m ? wave_min[w] : m;
    int32_t win = -1;
    if (m != ~0ull) {
      const uint32_t i = (uint32_t)(m & 0xFFFFFFFFull);
      const int32_t v = lb_out[(size_t)i * n_vars + var], cur = *best;
      if (mode == PCP_MINIMIZE ? v < cur : v > cur) {
        *best = v;
        if (improved) *improved += 1u;
        win = (int32_t)i;
      }
    }
    winner = win;
  }
  __syncthreads();
  const int32_t win = winner;
  if (win < 0) return;
  const size_t row = (size_t)win * n_vars;
  for (uint32_t j = threadIdx.x; j < n_vars; j += kReduceThreads) {
    if (best_lb) best_lb[j] = lb_out[row + j];
    if (best_ub) best_ub[j] = ub_out[row + j];
  }
  if (best_bits)
    for (uint32_t j = threadIdx.x; j < n_vars * set_words; j += kReduceThreads) best_bits[j] = bits_out[row * set_words + j];
}

}  // namespace

hipError_t launch_bnb_fold(uint32_t n_nodes, uint32_t n_vars, uint32_t var, uint32_t mode, const int32_t* best, int32_t* lb, int32_t* ub, uint64_t* bits,
                           uint32_t set_words, int32_t base, uint8_t* empty, hipStream_t stream) {
  hipLaunchKernelGGL(bnb_fold_kernel, dim3((n_nodes + kFoldThreads - 1) / kFoldThreads), dim3(kFoldThreads), 0, stream, n_nodes, n_vars, var, mode, best, lb, ub,
                     bits, set_words, base, empty);
  return hipGetLastError();
}

hipError_t launch_bnb_reduce(uint32_t n_nodes, uint32_t n_vars, uint32_t var, uint32_t mode, const uint8_t* empty, uint8_t* status, const int32_t* lb_out,
                             const int32_t* ub_out, const uint64_t* bits_out, uint32_t set_words, int32_t* best, int32_t* best_lb, int32_t* best_ub,
                             uint64_t* best_bits, uint32_t* improved, hipStream_t stream) {
  hipLaunchKernelGGL(bnb_reduce_kernel, dim3(1), dim3(kReduceThreads), 0, stream, n_nodes, n_vars, var, mode, empty, status, lb_out, ub_out, bits_out, set_words,
                     best, best_lb, best_ub, best_bits, improved);
  return hipGetLastError();
}

}  // namespace pcp
