// pcp_enum.hip — Brancher<FirstSmallestVar, MiddleVal | MinVal, Enumerate>::enter (search/branching/brancher.rs:52-71,
// search/branching/enumerate.rs:47-60) for every Unknown node of a propagated batch whose nodes carry value exclusions of their own
// (pcp_branch_device_excl).  The children are  x = v  and  x != v :  x = v  is folded into the bounds;  x != v  is folded when v is a bound of x
// (the propagator would fire once and be entailed) and otherwise becomes the entry (x, v) behind the exclusions the child inherits — those of
// the parent's entries whose value still lies inside their variable's domain in that child.  A value the node has excluded already is not
// chosen again: the nearest free value is taken, the lower one first.  The result is pcp_amd.search.branch_enumerate's, bit for bit.
//
// Four launches on the caller's stream, nothing synchronised:
//   branch_scan_kernel (pcp_kernels.hip)  statuses -> child slots in tree order, counts[0..5)
//   enum_select_kernel   one workgroup per Unknown node: the variable, the value, the number of entries each child keeps
//   enum_offsets_kernel  one workgroup: exclusive scan of those numbers in child ROW order -> child_excl_off, the total against the capacity
//   enum_write_kernel    one workgroup per Unknown node: the parent's row streamed into both children, the kept entries compacted in order
// An error (counts[6]) leaves the children unwritten: enum_write_kernel returns at once.
#include "pcp_internal.h"

namespace pcp {
namespace {

constexpr uint32_t kEnumBlock = 256;                   // threads per workgroup of the select and write kernels
constexpr uint32_t kEnumWaves = kEnumBlock / 64;
constexpr uint32_t kTakenWindow = 2048;                // distances from v covered by one pass of the taken bitmaps (one below v, one above)
constexpr uint32_t kNoVar = 0xFFFFFFFFu;

__device__ __forceinline__ unsigned long long block_min_u64(unsigned long long key, unsigned long long* sh) {
  for (int o = 32; o > 0; o >>= 1) key = min(key, (unsigned long long)__shfl_down(key, o));
  __syncthreads();  // (sh may still be read from the call before)
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = key;
  __syncthreads();
  key = sh[0];
  for (uint32_t w = 1; w < kEnumWaves; ++w) key = min(key, sh[w]);
  return key;
}

// Which children keep the entry (var, value) of a node branched on x with value v: bit 0 = the left child (x = v), bit 1 = the right child
// (x in [rl, ru]).  Any other variable has its parent's bounds in both children.  var >= n_vars is never used as an index: dropped.
__device__ __forceinline__ uint32_t enum_keep(uint32_t var, int32_t value, uint32_t n_vars, uint32_t x, int32_t v, int32_t rl, int32_t ru,
                                              const int32_t* __restrict__ plb, const int32_t* __restrict__ pub) {
  if (var >= n_vars) return 0u;
  if (var == x) return (value == v ? 1u : 0u) | ((value >= rl && value <= ru) ? 2u : 0u);
  return (value >= plb[var] && value <= pub[var]) ? 3u : 0u;
}

// x != v on [lo, hi]: folded into a bound when v is one (the lower bound first), else the bounds stay and the entry (x, v) is appended
__device__ __forceinline__ int32_t enum_right_lb(int32_t lo, int32_t v) { return v == lo ? v + 1 : lo; }
__device__ __forceinline__ int32_t enum_right_ub(int32_t lo, int32_t hi, int32_t v) { return (v != lo && v == hi) ? v - 1 : hi; }

__global__ void __launch_bounds__(kEnumBlock) enum_select_kernel(uint32_t n_vars, const int32_t* __restrict__ lb, const int32_t* __restrict__ ub,
                                                                 const uint32_t* __restrict__ child_base, const uint32_t* __restrict__ excl_off,
                                                                 const pcp_excl* __restrict__ excl, uint32_t val_mode, uint2* __restrict__ pick,
                                                                 uint32_t* __restrict__ cnt, uint32_t* __restrict__ counts, uint32_t var_select) {
  const uint32_t node = blockIdx.x, tid = threadIdx.x;
  const uint32_t slot = child_base[node];
  if (slot == kNoVar) return;  // not Unknown: nothing to branch on
  __shared__ unsigned long long sh64[kEnumWaves];
  __shared__ uint32_t taken[2][kTakenWindow / 32];  // [0]: values v - d, [1]: values v + d, bit d - d0
  __shared__ uint32_t shc[2][kEnumWaves];
  const int32_t* plb = lb + (size_t)node * n_vars;
  const int32_t* pub = ub + (size_t)node * n_vars;
  // FirstSmallestVar: minimum of (size << 32 | index) over the variables of size > 1 (first index wins ties), sizes in 64 bits; InputOrder
  // (input_order.rs:30-39): minimum of the index
  const uint32_t size_mask = var_size_mask(var_select);
  unsigned long long key = ~0ull;
  for (uint32_t i = tid; i < n_vars; i += kEnumBlock) {
    const unsigned long long size = (unsigned long long)((long long)pub[i] - (long long)plb[i] + 1);
    if (size > 1) key = min(key, var_key(size, i, size_mask));
  }
  key = block_min_u64(key, sh64);
  if (key == ~0ull) {
    // Unknown, yet no variable with more than one value: the reference panics here (first_smallest_var.rs:36)
    if (tid == 0) { pick[node] = make_uint2(kNoVar, 0u); cnt[slot] = 0u; cnt[slot + 1] = 0u; atomicMax(&counts[6], 3u); }
    return;
  }
  const uint32_t x = (uint32_t)key;
  const int32_t lo = plb[x], hi = pub[x];
  // MiddleVal: (lb + ub) / 2 on a 64-bit sum, C++ `/` truncates toward zero like Rust's (middle_val.rs:25-27); MinVal: lb (min_val.rs:25-27)
  long long v = val_mode == PCP_VAL_MIN ? (long long)lo : ((long long)lo + (long long)hi) / 2;
  const uint64_t e0 = excl_off ? excl_off[node] : 0u, e1 = excl_off ? excl_off[node + 1] : 0u;
  int hit = 0;
  for (uint64_t i = e0 + tid; i < e1; i += kEnumBlock) hit |= (excl[i].var == x && (long long)excl[i].value == v);
  if (__syncthreads_or(hit)) {
    // v is excluded already: the nearest value of [lo, hi] that is not, v - d before v + d.  The entries on x are marked in two bitmaps over the
    // distances [d0, d0 + kTakenWindow); a window without a free value holds that many entries, so k entries take at most k / kTakenWindow + 1 passes.
    const long long dmax = max(v - (long long)lo, (long long)hi - v);
    unsigned long long found = ~0ull;
    for (long long d0 = 1; d0 <= dmax; d0 += kTakenWindow) {
      for (uint32_t i = tid; i < 2 * (kTakenWindow / 32); i += kEnumBlock) (&taken[0][0])[i] = 0u;
      __syncthreads();
      for (uint64_t i = e0 + tid; i < e1; i += kEnumBlock) {
        if (excl[i].var != x) continue;
        const long long dist = (long long)excl[i].value - v, ad = dist < 0 ? -dist : dist;
        if (ad >= d0 && ad < d0 + (long long)kTakenWindow) atomicOr(&taken[dist > 0 ? 1 : 0][(uint32_t)(ad - d0) >> 5], 1u << ((uint32_t)(ad - d0) & 31u));
      }
      __syncthreads();
      unsigned long long k = ~0ull;
      for (uint32_t j = tid; j < kTakenWindow && k == ~0ull; j += kEnumBlock) {
        const long long d = d0 + j;
        const uint32_t bit = 1u << (j & 31u);
        if (v - d >= (long long)lo && !(taken[0][j >> 5] & bit)) k = 2ull * (unsigned long long)d;
        else if (v + d <= (long long)hi && !(taken[1][j >> 5] & bit)) k = 2ull * (unsigned long long)d + 1ull;
      }
      found = block_min_u64(k, sh64);
      if (found != ~0ull) break;
    }
    if (found == ~0ull) {
      // every value of x is excluded (the host brancher raises)
      if (tid == 0) { pick[node] = make_uint2(kNoVar, 0u); cnt[slot] = 0u; cnt[slot + 1] = 0u; atomicMax(&counts[6], 4u); }
      return;
    }
    const long long d = (long long)(found >> 1);
    v = (found & 1ull) ? v + d : v - d;
  }
  const int32_t vv = (int32_t)v;
  const int32_t rl = enum_right_lb(lo, vv), ru = enum_right_ub(lo, hi, vv);
  const bool append = vv != lo && vv != hi;
  uint32_t cl = 0, cr = 0;
  for (uint64_t i = e0 + tid; i < e1; i += kEnumBlock) {
    const uint32_t kb = enum_keep(excl[i].var, excl[i].value, n_vars, x, vv, rl, ru, plb, pub);
    cl += kb & 1u;
    cr += kb >> 1;
  }
  for (int o = 32; o > 0; o >>= 1) { cl += __shfl_down(cl, o); cr += __shfl_down(cr, o); }
  if ((tid & 63) == 0) { shc[0][tid >> 6] = cl; shc[1][tid >> 6] = cr; }
  __syncthreads();
  if (tid == 0) {
    cl = 0; cr = append ? 1u : 0u;
    for (uint32_t w = 0; w < kEnumWaves; ++w) { cl += shc[0][w]; cr += shc[1][w]; }
    pick[node] = make_uint2(x, (uint32_t)vv);
    cnt[slot] = cl;       // by child SLOT (tree order): the offsets kernel maps rows to slots
    cnt[slot + 1] = cr;
  }
}

// child_excl_off[r] = number of entries of the child rows before row r; row r is slot r, or slot n_children - 1 - r under branch_reverse.
__global__ void __launch_bounds__(1024) enum_offsets_kernel(const uint32_t* __restrict__ cnt, uint32_t* __restrict__ child_excl_off, uint32_t capacity,
                                                            uint32_t reverse, uint32_t* __restrict__ counts) {
  __shared__ unsigned long long wsum[16];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t n = counts[0];
  unsigned long long run = 0;
  for (uint32_t base = 0; base < n; base += 1024) {
    const uint32_t r = base + tid;
    const unsigned long long c = r < n ? cnt[reverse ? n - 1 - r : r] : 0u;
    unsigned long long inc = c;
    for (int o = 1; o < 64; o <<= 1) { const unsigned long long t = __shfl_up(inc, o); if ((int)lane >= o) inc += t; }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    unsigned long long before = 0, total = 0;
    for (uint32_t w = 0; w < 16; ++w) { if (w < wave) before += wsum[w]; total += wsum[w]; }
    if (r < n) child_excl_off[r] = (uint32_t)min(run + before + inc - c, 0xFFFFFFFFull);
    run += total;
    __syncthreads();
  }
  if (tid == 0) {
    child_excl_off[n] = (uint32_t)min(run, 0xFFFFFFFFull);
    counts[5] = (uint32_t)min(run, 0xFFFFFFFFull);
    if (run > (unsigned long long)capacity) atomicMax(&counts[6], 1u);
  }
}

__device__ __forceinline__ void set_lane(int4& q, uint32_t k, int32_t val) {
  q.x = k == 0 ? val : q.x; q.y = k == 1 ? val : q.y; q.z = k == 2 ? val : q.z; q.w = k == 3 ? val : q.w;
}

__global__ void __launch_bounds__(kEnumBlock) enum_write_kernel(uint32_t n_vars, const int32_t* __restrict__ lb, const int32_t* __restrict__ ub,
                                                                const uint32_t* __restrict__ child_base, const uint32_t* __restrict__ excl_off,
                                                                const pcp_excl* __restrict__ excl, const uint2* __restrict__ pick,
                                                                int32_t* __restrict__ child_lb, int32_t* __restrict__ child_ub, uint32_t* __restrict__ child_dirty,
                                                                const uint32_t* __restrict__ child_excl_off, pcp_excl* __restrict__ child_excl,
                                                                const uint32_t* __restrict__ counts, uint32_t reverse) {
  if (counts[6]) return;  // an error: the children are left unwritten (and no entry is written past the capacity)
  const uint32_t node = blockIdx.x, tid = threadIdx.x;
  const uint32_t slot = child_base[node];
  if (slot == kNoVar) return;
  // reverse: child k of the batch goes to row n_children-1-k (branch_kernel, pcp_kernels.hip)
  const uint32_t rowL = reverse ? counts[0] - 1 - slot : slot;
  const uint32_t rowR = reverse ? rowL - 1 : slot + 1;
  __shared__ uint32_t wt[2][kEnumWaves];
  const int32_t* plb = lb + (size_t)node * n_vars;
  const int32_t* pub = ub + (size_t)node * n_vars;
  const uint2 p = pick[node];
  const uint32_t x = p.x;
  const int32_t v = (int32_t)p.y;
  const int32_t lo = plb[x], hi = pub[x];
  const int32_t rl = enum_right_lb(lo, v), ru = enum_right_ub(lo, hi, v);
  const bool append = v != lo && v != hi;
  // the children differ from the parent's row — a fixpoint, if the caller propagated it — in this one variable (pcp_device_batch.dirty_var)
  if (child_dirty && tid == 0) { child_dirty[rowL] = x; child_dirty[rowR] = x; }
  int32_t* l0 = child_lb + (size_t)rowL * n_vars;
  int32_t* u0 = child_ub + (size_t)rowL * n_vars;
  int32_t* l1 = child_lb + (size_t)rowR * n_vars;
  int32_t* u1 = child_ub + (size_t)rowR * n_vars;
  // 16 bytes per lane when all six rows are 16-byte aligned, the rest of the row (or all of it) one int32 at a time
  const bool vec = (((uintptr_t)plb | (uintptr_t)pub | (uintptr_t)l0 | (uintptr_t)u0 | (uintptr_t)l1 | (uintptr_t)u1) & 15u) == 0;
  const uint32_t nq = vec ? n_vars >> 2 : 0u;
  for (uint32_t q = tid; q < nq; q += kEnumBlock) {
    const int4 a = reinterpret_cast<const int4*>(plb)[q], b = reinterpret_cast<const int4*>(pub)[q];
    int4 al = a, bl = b, ar = a, br = b;
    if ((x >> 2) == q) { set_lane(al, x & 3u, v); set_lane(bl, x & 3u, v); set_lane(ar, x & 3u, rl); set_lane(br, x & 3u, ru); }
    reinterpret_cast<int4*>(l0)[q] = al;
    reinterpret_cast<int4*>(u0)[q] = bl;
    reinterpret_cast<int4*>(l1)[q] = ar;
    reinterpret_cast<int4*>(u1)[q] = br;
  }
  for (uint32_t i = 4u * nq + tid; i < n_vars; i += kEnumBlock) {
    const int32_t a = plb[i], b = pub[i];
    l0[i] = (i == x) ? v : a;   // left:  x = v
    u0[i] = (i == x) ? v : b;
    l1[i] = (i == x) ? rl : a;  // right: x != v, folded when v is a bound
    u1[i] = (i == x) ? ru : b;
  }
  // the kept entries, in the parent's order: ballot + popcount per wavefront, the wavefronts' totals through LDS, a running base across chunks
  const uint64_t e0 = excl_off ? excl_off[node] : 0u, e1 = excl_off ? excl_off[node + 1] : 0u;
  pcp_excl* outL = child_excl + child_excl_off[rowL];
  pcp_excl* outR = child_excl + child_excl_off[rowR];
  const uint32_t lane = tid & 63, wave = tid >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  uint32_t baseL = 0, baseR = 0;
  for (uint64_t cb = e0; cb < e1; cb += kEnumBlock) {
    const uint64_t i = cb + tid;
    uint32_t ev = 0, kb = 0;
    int32_t ew = 0;
    if (i < e1) { ev = excl[i].var; ew = excl[i].value; kb = enum_keep(ev, ew, n_vars, x, v, rl, ru, plb, pub); }
    const unsigned long long mL = __ballot(kb & 1u), mR = __ballot(kb & 2u);
    if (lane == 0) { wt[0][wave] = (uint32_t)__popcll(mL); wt[1][wave] = (uint32_t)__popcll(mR); }
    __syncthreads();
    uint32_t pL = baseL + (uint32_t)__popcll(mL & below), pR = baseR + (uint32_t)__popcll(mR & below), tL = 0, tR = 0;
    for (uint32_t w = 0; w < kEnumWaves; ++w) {
      if (w < wave) { pL += wt[0][w]; pR += wt[1][w]; }
      tL += wt[0][w]; tR += wt[1][w];
    }
    if (kb & 1u) { outL[pL].var = ev; outL[pL].value = ew; }
    if (kb & 2u) { outR[pR].var = ev; outR[pR].value = ew; }
    baseL += tL; baseR += tR;
    __syncthreads();
  }
  if (append && tid == 0) { outR[baseR].var = x; outR[baseR].value = v; }  // the new entry comes last
}

}  // namespace

hipError_t launch_enum_branch(uint32_t n_nodes, uint32_t n_vars, const int32_t* lb, const int32_t* ub, const uint32_t* child_base, const uint32_t* excl_off,
                              const pcp_excl* excl, uint32_t val, uint2* pick, uint32_t* cnt, int32_t* child_lb, int32_t* child_ub, uint32_t* child_dirty,
                              uint32_t* child_excl_off, pcp_excl* child_excl, uint32_t child_excl_capacity, uint32_t* counts, uint32_t reverse,
                              uint32_t var_select, hipStream_t stream) {
  hipLaunchKernelGGL(enum_select_kernel, dim3(n_nodes), dim3(kEnumBlock), 0, stream, n_vars, lb, ub, child_base, excl_off, excl, val, pick, cnt, counts, var_select);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(enum_offsets_kernel, dim3(1), dim3(1024), 0, stream, cnt, child_excl_off, child_excl_capacity, reverse, counts);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(enum_write_kernel, dim3(n_nodes), dim3(kEnumBlock), 0, stream, n_vars, lb, ub, child_base, excl_off, excl, pick, child_lb, child_ub,
                     child_dirty, child_excl_off, child_excl, counts, reverse);
  return hipGetLastError();
}

}  // namespace pcp
