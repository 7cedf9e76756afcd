// pcp_setform.hip — the propagation fixpoint of stores that hold FORMULA propagators (the reified layer, logic/) over IntervalSet<i32>
// domains: pcp_formula.hip's trees of Conjunction / Disjunction nodes over elementary leaves, evaluated on pcp_set.hip's bit sets.  gfx950.
//
// The reference's reified layer is generic in the domain (logic/*.rs are written against the Subsumption / Propagator traits only), and its
// default space FDSpace holds IntervalSet domains (variable/mod.rs:38, search/mod.rs:41-43): over sets a leaf's is_subsumed() sees more than
// over intervals — XEqY is disentailed as soon as the two SETS are disjoint, whatever their hulls (x_eq_y.rs:87-93 through
// IntervalSet::is_disjoint) — so a Disjunction unit-propagates earlier and the fixpoints differ from interval mode's.
//
// MI355X mapping, as formfix_kernel: one WAVEFRONT per node, up to four per workgroup, persistent workgroups; one lane per unit
// (lane-strided beyond 64 units); a unit's tree walked by two loops over its breadth-first node array with 64-bit true / false / active
// masks; rounds until a round narrows nothing.  The node lives in the wavefront's LDS slice as in setfix_kernel:
//   bits[V][set_words] u64   value v of variable x <-> bit (v - base) of bits[x]; narrowing = ds_and_b64 (SetDomT, pcp_setdom.hpp)
//   bnd[V] (lb, ub)          the sets' bounds, re-derived at the start of a round for the variables the round before marked changed
// Parity with the reference's FIFO (DESIGN.md §2 "Formula units" and "Set mode"): the filters are monotone and contracting;
// is_subsumed() only moves from Unknown to True or False as sets shrink, so a decision taken on an older set is the conservative one and
// the next round repeats it; between two bounds steps a cached bound is a superset read.  The last round narrows nothing, so it has seen
// exact bounds and final sets throughout.
// These stores are small and branchy: the kernel is written for correctness and occupancy of the chip by nodes, not for bandwidth.
#include <algorithm>

#include "pcp_setform.hpp"  // setform_carve, the leaves and the unit step, shared with pcp_setformdfs.hip

namespace pcp {

namespace {

// See the head of the file.  IMPLICIT: no `active` rows are read, every unit starts live (liveness is derived: an entailed unit is unlinked
// in either mode — its propagate() is a no-op from then on, disjunction.rs:103); rows are written when active_out is given.
template <bool IMPLICIT>
__global__ void __launch_bounds__(256) setformfix_kernel(const SetFormArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6), nwv = blockDim.x >> 6;
  const uint32_t V = a.m.n_vars, sw = a.set_words, Wv = (V + 31) >> 5, U = a.n_units, Wu = (U + 31) >> 5;
  const SetFormCarve cv = setform_carve(V, sw, U);
  unsigned char* const mine = smem + (size_t)wv * cv.total;
  unsigned long long* const bits = reinterpret_cast<unsigned long long*>(mine + cv.bits);
  int2* const bnd = reinterpret_cast<int2*>(mine + cv.bnd);
  uint32_t* const chg = reinterpret_cast<uint32_t*>(mine + cv.chg);
  uint32_t* const live = reinterpret_cast<uint32_t*>(mine + cv.live);
  uint32_t* const misc = reinterpret_cast<uint32_t*>(mine + cv.misc);
  const uint32_t words64 = (U + 63) >> 6, nwords = V * sw;
  auto wave_sync = [] { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier(); };
  pcp_stats* const stats = a.stats + (blockIdx.x & (kStatSlots - 1));
  unsigned long long acc_s2 = 0, acc_s3 = 0, acc_narrow = 0, acc_waves = 0, acc_nodes = 0, acc_failed = 0;

  for (uint32_t node = blockIdx.x * nwv + wv; node < a.n_nodes; node += gridDim.x * nwv) {
    const size_t row = (size_t)node * V;
    if (lane < 32u) misc[lane] = 0;
    for (uint32_t w = lane; w < Wv; w += 64) chg[w] = 0;
    // Store::active (one bit per unit): the caller's row, or every unit
    for (uint32_t w = lane; w < Wu; w += 64) {
      uint32_t lv = 0xFFFFFFFFu;
      if constexpr (!IMPLICIT) {
        if (a.active_in) { const uint64_t q = a.active_in[(size_t)node * words64 + (w >> 1)]; lv = (uint32_t)(q >> (32 * (w & 1))); }
      }
      if (w == Wu - 1 && (U & 31u)) lv &= (1u << (U & 31u)) - 1u;
      live[w] = lv;
    }
    {
      const uint64_t* src = a.bits_in + row * sw;
      for (uint32_t i = lane; i < nwords; i += 64) bits[i] = src[i];
    }
    wave_sync();
    bool bad = false;
    for (uint32_t v = lane; v < V; v += 64) {
      const int2 b = scan_bounds(bits + (size_t)v * sw, sw, a.base);
      bnd[v] = b;
      bad |= b.x > b.y;  // an empty input domain
    }
    if (__ballot(bad) && lane == 0) misc[S_FAIL] = 1u;
    wave_sync();

    uint32_t narrow = 0, steps2 = 0, steps3 = 0, rounds = 0;
    const SetDom dm{bits, bnd, a.m.const_val, V, sw, a.base, chg, misc, &narrow};
    bool failed = __builtin_amdgcn_readfirstlane(misc[S_FAIL]) != 0;
    while (!failed) {
      ++rounds;
      if (rounds > 1) {
        // the exact bounds of every variable the round before narrowed, from its words; an emptied set fails the node
        bool emptied = false;
        for (uint32_t v = lane; v < V; v += 64) {
          if (!((chg[v >> 5] >> (v & 31u)) & 1u)) continue;
          const int2 b = scan_bounds(bits + (size_t)v * sw, sw, a.base);
          bnd[v] = b;
          emptied |= b.x > b.y;
        }
        wave_sync();
        for (uint32_t w = lane; w < Wv; w += 64) chg[w] = 0;
        wave_sync();
        if (__ballot(emptied)) { failed = true; break; }
      }
      const uint32_t before = narrow;
      for (uint32_t u = lane; u < U; u += 64) {
        if (!((live[u >> 5] >> (u & 31u)) & 1u)) continue;
        const bool entailed = setform_unit_step(a.nodes, a.unit_root, a.m.recs, u, dm, steps2, steps3);
        if (entailed) atomicAnd(&live[u >> 5], ~(1u << (u & 31u)));      // unlink_prop (store.rs:200-207)
      }
      wave_sync();
      failed = __builtin_amdgcn_readfirstlane(misc[S_FAIL]) != 0;
      if (!__ballot(narrow != before)) break;
    }

    // ---- write back -----------------------------------------------------------------------------------------------------------------
    {
      uint64_t* dst = a.bits_out + row * sw;
      for (uint32_t i = lane; i < nwords; i += 64) dst[i] = bits[i];
    }
    for (uint32_t v = lane; v < V; v += 64) {
      const int2 b = bnd[v];
      a.lb_out[row + v] = b.x; a.ub_out[row + v] = b.y;
    }
    bool any_live = false;
    for (uint32_t w = lane; w < Wu; w += 64) any_live |= live[w] != 0;
    if (a.active_out)
      for (uint32_t w = lane; w < words64; w += 64) {
        const uint64_t lo = live[2 * w], hi = (2 * w + 1 < Wu) ? live[2 * w + 1] : 0u;
        a.active_out[(size_t)node * words64 + w] = lo | (hi << 32);
      }
    const bool unknown = __ballot(any_live) != 0;
    // Consistency::consistency (store.rs:250-256): False if a propagate failed, True if no subscription remains, else Unknown
    if (lane == 0) a.status[node] = failed ? (uint8_t)PCP_FALSE : (unknown ? (uint8_t)PCP_UNKNOWN : (uint8_t)PCP_TRUE);
    for (int o = 32; o > 0; o >>= 1) { steps2 += __shfl_down(steps2, o); steps3 += __shfl_down(steps3, o); narrow += __shfl_down(narrow, o); }
    acc_s2 += steps2; acc_s3 += steps3; acc_narrow += narrow; acc_waves += rounds ? rounds : 1; acc_nodes += 1; acc_failed += failed ? 1 : 0;
    wave_sync();
  }
  if (lane == 0) {
    if (acc_s2) atomicAdd((unsigned long long*)&stats->steps, acc_s2);
    if (acc_s3) atomicAdd((unsigned long long*)&stats->steps3, acc_s3);
    if (acc_s2 + acc_s3) { atomicAdd((unsigned long long*)&stats->evaluated, acc_s2 + acc_s3); atomicAdd((unsigned long long*)&stats->full_evals, acc_s2 + acc_s3); }
    if (acc_narrow) atomicAdd((unsigned long long*)&stats->narrowings, acc_narrow);
    if (acc_waves) atomicAdd((unsigned long long*)&stats->waves, acc_waves);
    if (acc_nodes) atomicAdd((unsigned long long*)&stats->nodes, acc_nodes);
    if (acc_failed) atomicAdd((unsigned long long*)&stats->failed_nodes, acc_failed);
  }
}

}  // namespace

size_t lds_bytes_setform(uint32_t n_vars, uint32_t set_words, uint32_t n_units, uint32_t waves) {
  const SetFormCarve c = setform_carve(n_vars, set_words, n_units);
  return c.total * waves <= 160 * 1024 ? c.total * waves : 0;
}

hipError_t launch_setformfix(const SetFormArgs& a, bool implicit, const LaunchPlan& p, hipStream_t stream) {
  const void* fn = implicit ? reinterpret_cast<const void*>(setformfix_kernel<true>) : reinterpret_cast<const void*>(setformfix_kernel<false>);
  if (p.lds_bytes > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes);
    if (e != hipSuccess) return e;
  }
  if (implicit) hipLaunchKernelGGL(setformfix_kernel<true>, dim3(p.grid), dim3(p.block), p.lds_bytes, stream, a);
  else hipLaunchKernelGGL(setformfix_kernel<false>, dim3(p.grid), dim3(p.block), p.lds_bytes, stream, a);
  return hipGetLastError();
}

}  // namespace pcp
