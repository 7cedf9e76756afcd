// pcp_formula.hip — the propagation fixpoint of stores that hold FORMULA propagators (the reified layer, logic/): units that are
// trees of Conjunction (logic/conjunction.rs:77-119) and Disjunction (logic/disjunction.rs:78-141) nodes over elementary leaves,
// Boolean / BooleanNeg (logic/boolean.rs:111-140, logic/boolean_neg.rs:71-96) among them — what implication / equivalence
// (logic/mod.rs:30-45) and propagators::Cumulative::join (propagators/cumulative.rs:59-114) allocate.  gfx950.
//
// Same contract as the other fixpoint kernels: Store::consistency (propagation/store.rs:125-164, 247-257) for a batch of nodes,
// explicit `active` rows (one bit per UNIT) or implicit-active nodes.  What is new is that a pop of a unit is not a filter but a
// small program: Disjunction::propagate first asks every child for is_subsumed() and propagates a child only when it is the
// single one left that is not disentailed (unit propagation, disjunction.rs:97-117); Conjunction::propagate runs its children in
// order.  Every unit of such a store — formula or not — is held as a tree here (a standalone propagator is a tree of one leaf,
// a Conjunction / Distinct group an AND over its members), and ONE LANE evaluates one unit.
//
// MI355X mapping: one workgroup of 256 threads per node; the node's domains in LDS as (-lb, ub) cells (LdsDom, narrowing =
// ds_min); a round = every live unit once, lane-strided; rounds until a round narrows nothing (Jacobi waves: the filters are
// monotone and contracting, is_subsumed() only moves from Unknown to True or False as domains shrink, so a decision taken on a
// stale domain is a conservative one that the next round repeats — same fixpoint as the reference's FIFO).  An
// entailed unit is unlinked (store.rs:200-207) — in implicit mode too: its propagate() is a no-op from then on.
// These stores are small and branchy (15 units for three tasks): the kernel is written for correctness and occupancy of the
// chip by nodes, not for bandwidth; no MFMA, no bulk tests.
#include <algorithm>

#include "pcp_formula.hpp"

namespace pcp {

// One WAVEFRONT per node (round 4; it was a 256-thread workgroup per node with one lane per unit and the tree walked by recursion unrolled
// eight levels deep: 178 VGPRs, 256 bytes of scratch per lane).  One LANE runs one unit: form_unit_step (pcp_formula.hpp), two loops over the
// unit's nodes instead of the recursion; formdfs_kernel (pcp_formdfs.hip) takes the same step inside its search loop.
__global__ void __launch_bounds__(256) formfix_kernel(const FormArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6), nwv = blockDim.x >> 6;
  const uint32_t V = a.m.n_vars, S = a.m.n_slots, Wv = (S + 31) >> 5, U = a.n_units, Wu = (U + 31) >> 5;
  const FormCarve cv = form_carve(S, U);
  unsigned char* const mine = smem + (size_t)wv * cv.total;
  int2* const dom = reinterpret_cast<int2*>(mine + cv.dom);
  uint32_t* const chg = reinterpret_cast<uint32_t*>(mine + cv.chg);
  uint32_t* const live = reinterpret_cast<uint32_t*>(mine + cv.live);
  uint32_t* const misc = reinterpret_cast<uint32_t*>(mine + cv.misc);
  const uint32_t words64 = (U + 63) >> 6;
  auto wave_sync = [] { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier(); };
  pcp_stats* const stats = a.stats + (blockIdx.x & (kStatSlots - 1));
  unsigned long long acc_s2 = 0, acc_s3 = 0, acc_narrow = 0, acc_waves = 0, acc_nodes = 0, acc_failed = 0;

  uint32_t n_nodes = a.n_nodes, st_base = 0;
  size_t row_base = 0;
  if (a.sp_ptr) {  // host-stepped device-side DFS (pcp_dfs_device): ONE node, the one on top of the stack
    const uint32_t sp = *a.sp_ptr;
    if (sp == 0 || *a.stop_ptr) return;
    row_base = (size_t)(sp - 1) * V; st_base = sp - 1; n_nodes = 1;
  }
  for (uint32_t node = blockIdx.x * nwv + wv; node < n_nodes; node += gridDim.x * nwv) {
    const size_t row = row_base + (size_t)node * V;
    if (lane < (uint32_t)F_WORDS) misc[lane] = 0;
    for (uint32_t w = lane; w < Wv; w += 64) chg[w] = 0;
    // Store::active (one bit per unit): the caller's row, or every unit (implicit-active nodes)
    for (uint32_t w = lane; w < Wu; w += 64) {
      uint32_t bits = 0xFFFFFFFFu;
      if (a.active_in) { const uint64_t q = a.active_in[(size_t)node * words64 + (w >> 1)]; bits = (uint32_t)(q >> (32 * (w & 1))); }
      if (w == Wu - 1 && (U & 31u)) bits &= (1u << (U & 31u)) - 1u;
      live[w] = bits;
    }
    bool bad = false, wide = false;
    for (uint32_t v = lane; v < S; v += 64) {
      int l = 0, u = 0;
      if (v < V) {
        l = a.lb_in[row + v]; u = a.ub_in[row + v];
        bad |= l > u;
        wide |= (l < -kBoundMax) | (l > kBoundMax) | (u < -kBoundMax) | (u > kBoundMax);
      } else if (v - V >= a.m.sums.count) {
        l = u = a.m.const_val[v - V];  // (the Sum slots in between hold nothing: their domain is computed from the members)
      }
      dom[v] = make_int2(-l, u);
    }
    if (__ballot(wide)) {  // a bound beyond +-(2^29 - 1): refused, not wrapped (pcp_hip.h)
      if (lane == 0) { a.status[st_base + node] = kStatusRetry; atomicMax(a.violation, 1u); }
      continue;
    }
    if (__ballot(bad) && lane == 0) misc[F_FAIL] = 1u;
    wave_sync();

    Ctr ctr;
    const LdsDom dm{dom, 1u, chg, &misc[F_FAIL], 1u, &ctr, a.m.sums};
    uint32_t steps2 = 0, steps3 = 0, rounds = 0;
    bool failed = __builtin_amdgcn_readfirstlane(misc[F_FAIL]) != 0;
    while (!failed) {
      ++rounds;
      const uint32_t before = ctr.narrow;
      for (uint32_t u = lane; u < U; u += 64) {
        if (!((live[u >> 5] >> (u & 31u)) & 1u)) continue;
        const bool entailed = form_unit_step(a.nodes, a.unit_root, a.m.recs, u, dm, steps2, steps3);
        if (entailed) atomicAnd(&live[u >> 5], ~(1u << (u & 31u)));      // unlink_prop (store.rs:200-207)
      }
      wave_sync();
      failed = __builtin_amdgcn_readfirstlane(misc[F_FAIL]) != 0;
      if (!__ballot(ctr.narrow != before)) break;
    }

    // ---- write back -----------------------------------------------------------------------------------------------------------------
    bool emptied = false;
    for (uint32_t v = lane; v < V; v += 64) {
      const int2 d = dom[v];
      emptied |= -d.x > d.y;
      a.lb_out[row + v] = -d.x; a.ub_out[row + v] = d.y;
    }
    failed = failed || __ballot(emptied) != 0;
    bool any_live = false;
    for (uint32_t w = lane; w < Wu; w += 64) any_live |= live[w] != 0;
    if (a.active_out)
      for (uint32_t w = lane; w < words64; w += 64) {
        const uint64_t lo = live[2 * w], hi = (2 * w + 1 < Wu) ? live[2 * w + 1] : 0u;
        a.active_out[(size_t)node * words64 + w] = lo | (hi << 32);
      }
    const bool unknown = __ballot(any_live) != 0;
    // Consistency::consistency (store.rs:250-256): False if a propagate failed, True if no subscription remains, else Unknown
    if (lane == 0) a.status[st_base + node] = failed ? (uint8_t)PCP_FALSE : (unknown ? (uint8_t)PCP_UNKNOWN : (uint8_t)PCP_TRUE);
    for (int o = 32; o > 0; o >>= 1) { steps2 += __shfl_down(steps2, o); steps3 += __shfl_down(steps3, o); ctr.narrow += __shfl_down(ctr.narrow, o); }
    acc_s2 += steps2; acc_s3 += steps3; acc_narrow += ctr.narrow; acc_waves += rounds ? rounds : 1; acc_nodes += 1; acc_failed += failed ? 1 : 0;
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

size_t lds_bytes_formula(uint32_t n_slots, uint32_t n_units, uint32_t waves) {
  const FormCarve c = form_carve(n_slots, n_units);
  return c.total * waves <= 160 * 1024 ? c.total * waves : 0;
}

hipError_t launch_formfix(const FormArgs& a, const LaunchPlan& p, hipStream_t stream) {
  if (p.lds_bytes > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(formfix_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(formfix_kernel, dim3(p.grid), dim3(p.block), p.lds_bytes, stream, a);
  return hipGetLastError();
}

}  // namespace pcp
