// pcp_steal.hip — pcp_dfs_forest_steal: between two launches of an Interval forest, idle trees take the BOTTOM row of trees that have two or
// more open nodes, on the device.  Three kernels on one stream, so that stream order is the only synchronisation there is:
//   steal_verdict_kernel   one thread per pair: is the pair valid on the state as the call found it?  It writes done[] and nothing else, so
//                          no pair's verdict can depend on another pair;
//   steal_move_kernel      pairs x column slices, one wavefront each.  A slice of the stack's columns (lb and ub side by side) hands row 0
//                          to the receiver and shifts the donor's rows down by one: the thread that owns a column loads [r + 1] and then
//                          stores [r] for rising r, which needs no barrier and no second buffer.  One more block per pair does the same for
//                          the one-word-per-row arrays (dirty, row_base, row_excl) and copies the path prefix.  Only pairs with done == 1
//                          are touched; sp is read, never written;
//   steal_commit_kernel    one thread per pair: sp[donor] -= 1, sp[receiver] = 1.
// Every index that addresses memory comes from a pair the verdict kernel accepted: both trees < n_trees, 2 <= sp[donor] <= capacity,
// row_base[donor][0] <= path_capacity.
#include "pcp_internal.h"

namespace pcp {

namespace {

constexpr uint32_t kStealThreads = 64;  // one wavefront per block: a pair's slices spread over the CUs
constexpr uint32_t kStealUnroll = 8;    // rows a thread keeps in flight: the shift is a chain of load [r + 1] -> store [r]
typedef int32_t Row16 __attribute__((ext_vector_type(4)));  // four words of a row, moved as one 16-byte access (a plain vector: it stays in registers)
constexpr uint32_t kStealMaxSlices = 4096;  // grid.y stays far below its limit of 65 535

__global__ void __launch_bounds__(256) steal_verdict_kernel(const StealArgs a, const uint32_t* __restrict__ pairs, uint32_t* __restrict__ done) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n_pairs) return;
  const uint32_t d = pairs[2 * (size_t)i], r = pairs[2 * (size_t)i + 1];
  bool ok = d != r && d < a.n_trees && r < a.n_trees;
  if (ok) {
    const uint32_t k = a.sp[d];
    ok = a.sp[r] == 0 && k >= 2 && k <= a.capacity;
  }
  if (ok && a.row_base) ok = a.row_base[(size_t)d * a.capacity] <= a.path_capacity;
  done[i] = ok ? 1u : 0u;
}

// Column `col` of a stack of k rows (`stride` elements apart): row 0 goes to the receiver, rows 1 .. k-1 move down by one.
template <typename T>
__device__ __forceinline__ void shift_column(T* __restrict__ dst0, T* src, size_t stride, uint32_t k) {
  *dst0 = *src;
  uint32_t r = 0;
  for (; r + kStealUnroll < k; r += kStealUnroll) {
    T v[kStealUnroll];
#pragma unroll
    for (uint32_t j = 0; j < kStealUnroll; ++j) v[j] = src[(size_t)(r + 1 + j) * stride];
#pragma unroll
    for (uint32_t j = 0; j < kStealUnroll; ++j) src[(size_t)(r + j) * stride] = v[j];
  }
  for (; r + 1 < k; ++r) src[(size_t)r * stride] = src[(size_t)(r + 1) * stride];
}

// A one-word-per-row array of k rows shared by the block's threads: chunks of blockDim rows, every thread loads [base + tid + 1], the
// barrier, then stores [base + tid].  A chunk's stores end below the next chunk's loads, and the one element two chunks share is loaded
// before the barrier the storing thread has to pass.
template <typename T>
__device__ __forceinline__ void shift_rows(T* rows, uint32_t k) {
  for (uint32_t base = 0; base + 1 < k; base += blockDim.x) {  // (block-uniform bounds: every thread reaches every barrier)
    const uint32_t r = base + threadIdx.x;
    const bool mine = r + 1 < k;
    T v{};
    if (mine) v = rows[r + 1];
    __syncthreads();
    if (mine) rows[r] = v;
  }
}

template <bool VEC>
__global__ void __launch_bounds__(kStealThreads) steal_move_kernel(const StealArgs a, const uint32_t* __restrict__ pairs, const uint32_t* __restrict__ done) {
  const uint32_t i = blockIdx.x;
  if (!done[i]) return;  // (block-uniform)
  const uint32_t d = pairs[2 * (size_t)i], r = pairs[2 * (size_t)i + 1];
  const uint32_t k = a.sp[d], V = a.n_vars, cap = a.capacity;
  const size_t tree = (size_t)cap * V;
  if (blockIdx.y < a.col_slices) {
    // columns [0, W) are lb's, [W, 2 W) ub's; W = V words, or V / 4 16-byte vectors when the base and the row stride keep them aligned
    const uint32_t W = VEC ? V / 4 : V;
    for (uint32_t col = blockIdx.y * kStealThreads + threadIdx.x; col < 2 * W; col += a.col_slices * kStealThreads) {  // (one turn unless the row is very wide)
      int32_t* const arr = col < W ? a.lb : a.ub;
      const uint32_t c = col < W ? col : col - W;
      if (VEC) shift_column(reinterpret_cast<Row16*>(arr + (size_t)r * tree) + c, reinterpret_cast<Row16*>(arr + (size_t)d * tree) + c, V / 4, k);
      else shift_column(arr + (size_t)r * tree + c, arr + (size_t)d * tree + c, V, k);
    }
    return;
  }
  // the rows' words: the receiver's row 0 and its path prefix first (they read the donor's row 0), then the donor's rows move down
  if (a.row_base) {
    const uint32_t nb = a.row_base[(size_t)d * cap];
    const pcp_excl* const ps = a.path + (size_t)d * a.path_capacity;
    pcp_excl* const pd = a.path + (size_t)r * a.path_capacity;
    for (uint32_t e = threadIdx.x; e < nb; e += blockDim.x) pd[e] = ps[e];  // (nb <= path_capacity; nb == 0 with a null path)
    if (threadIdx.x == 0) {
      a.row_base[(size_t)r * cap] = nb;
      a.row_excl[(size_t)r * cap] = a.row_excl[(size_t)d * cap];
    }
  }
  if (a.dirty && threadIdx.x == 0) a.dirty[(size_t)r * cap] = a.dirty[(size_t)d * cap];
  __syncthreads();
  if (a.dirty) shift_rows(a.dirty + (size_t)d * cap, k);
  if (a.row_base) {
    shift_rows(a.row_base + (size_t)d * cap, k);
    shift_rows(a.row_excl + (size_t)d * cap, k);
  }
}

__global__ void __launch_bounds__(256) steal_commit_kernel(const StealArgs a, const uint32_t* __restrict__ pairs, const uint32_t* __restrict__ done) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n_pairs || !done[i]) return;
  a.sp[pairs[2 * (size_t)i]] -= 1;
  a.sp[pairs[2 * (size_t)i + 1]] = 1;
}

}  // namespace

hipError_t launch_forest_steal(const StealArgs& args, const uint32_t* pairs, uint32_t* done, hipStream_t stream) {
  if (!args.n_pairs) return hipSuccess;
  StealArgs a = args;
  const uint32_t V = a.n_vars;
  // 16-byte accesses only where every row of both arrays starts on a 16-byte boundary: a row is V words behind the array's base
  const bool vec = V % 4 == 0 && ((reinterpret_cast<uintptr_t>(a.lb) | reinterpret_cast<uintptr_t>(a.ub)) & 15u) == 0;
  const uint32_t cols = 2 * (vec ? V / 4 : V);
  a.col_slices = (cols + kStealThreads - 1) / kStealThreads;
  if (a.col_slices > kStealMaxSlices) a.col_slices = kStealMaxSlices;  // (a slice then owns several columns per thread)
  const uint32_t flat = (a.n_pairs + 255) / 256;
  hipLaunchKernelGGL(steal_verdict_kernel, dim3(flat), dim3(256), 0, stream, a, pairs, done);
  const dim3 grid(a.n_pairs, a.col_slices + 1);  // (+ 1: the block of the rows' words)
  if (vec) hipLaunchKernelGGL(steal_move_kernel<true>, grid, dim3(kStealThreads), 0, stream, a, pairs, done);
  else hipLaunchKernelGGL(steal_move_kernel<false>, grid, dim3(kStealThreads), 0, stream, a, pairs, done);
  hipLaunchKernelGGL(steal_commit_kernel, dim3(flat), dim3(256), 0, stream, a, pairs, done);
  return hipGetLastError();
}

}  // namespace pcp
