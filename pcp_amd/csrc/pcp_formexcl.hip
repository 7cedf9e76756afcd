// pcp_formexcl.hip — the propagation fixpoint of stores WITH FORMULA UNITS whose nodes carry VALUE EXCLUSIONS of their own, optionally under
// branch and bound (gfx950): pcp_propagate_device_form_excl.  To formfix_kernel (pcp_formula.hip) what smallexcl_kernel (pcp_smallexcl.hip) is to
// smallfix_kernel: the companion for what a brancher writes.
//
// Enumerate's right branch  x != v  (search/branching/enumerate.rs:54-59) over an Interval removes a value only at a bound (x_neq_y.rs:82-93):
// with v inside the domain it removes nothing and stays in that ONE node's cstore until v reaches a bound.  pcp_branch_device_excl writes such
// propagators as 8-byte pcp_excl entries, a CSR slice per node.  A schedule (propagators::Cumulative::join, cumulative.rs:59-114) is a store of
// formula units, which neither pcp_propagate_device_excl nor pcp_propagate_device_small_excl takes; this kernel sweeps the entries next to the trees.
//
// MI355X mapping: formfix_kernel's — ONE WAVEFRONT PER NODE, four nodes per 256-thread workgroup, the node's (-lb, ub) cells in the wavefront's
// LDS slice (form_carve), one lane per unit (form_unit_step, pcp_formula.hpp), rounds separated by the wavefront barrier + fence.  At the top of
// EVERY round the wavefront sweeps the node's slice excl[excl_off[i] .. excl_off[i + 1]) lane-strided from global memory (the lists belong to
// one node each: nothing to share in LDS):  XNeqY(Identity(var), Constant(value))::propagate, then is_subsumed() on what it left
// (store.rs:166-175) — entailed iff the value lies outside [lb, ub]; an exclusion that is not entailed keeps the node PCP_UNKNOWN.  A wavefront
// barrier, then every live unit once.  The exclusions are monotone contracting filters like the leaves of the trees, and a formula decision on
// a domain an exclusion has since narrowed is the conservative one the next round repeats: the fixpoint is the reference's.
// Nodes are implicit (every unit live on entry); there is no device DFS stack here.
//
// BNB = true: BranchAndBound's bound propagator (search/branch_and_bound.rs:64-84: var < best / var > best once a solution is known) narrows
// its variable once and is then entailed, so it is folded into the objective's cell WHILE THE NODE IS STAGED — no launch in front of the
// fixpoint.  A node the fold would empty comes out PCP_FALSE with its row as it went in and is marked in the context's `empty` scratch, so
// that bnb_reduce_kernel (pcp_bnb.hip) runs behind this launch as it does behind bnb_fold_kernel + any fixpoint.  Vector memory operations only.
#include "pcp_formula.hpp"

namespace pcp {

template <bool BNB>
__global__ void __launch_bounds__(256) formexcl_kernel(const FormExclArgs x) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const FormArgs& a = x.f;
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
  // the incumbent as it stands when the launch starts (bnb_reduce_kernel replaces it behind the launch): lane 0's read, for the wavefront
  int best = 0;
  if (BNB) { if (lane == 0) best = *x.obj_best; best = __builtin_amdgcn_readfirstlane(best); }

  const uint32_t n_nodes = a.n_nodes;
  for (uint32_t node = blockIdx.x * nwv + wv; node < n_nodes; node += gridDim.x * nwv) {
    const size_t row = (size_t)node * V;
    // ---- stage: the node's domains (the objective's cell folded against the incumbent), every unit live ---------------------------------------
    if (lane < (uint32_t)F_WORDS) misc[lane] = 0;
    for (uint32_t w = lane; w < Wv; w += 64) chg[w] = 0;
    for (uint32_t w = lane; w < Wu; w += 64) {
      uint32_t bits = 0xFFFFFFFFu;
      if (w == Wu - 1 && (U & 31u)) bits &= (1u << (U & 31u)) - 1u;
      live[w] = bits;
    }
    bool bad = false, wide = false, fold_empty = false;
    for (uint32_t v = lane; v < S; v += 64) {
      int l = 0, u = 0;
      if (v < V) {
        l = a.lb_in[row + v]; u = a.ub_in[row + v];
        bad |= l > u;
        wide |= (l < -kBoundMax) | (l > kBoundMax) | (u < -kBoundMax) | (u > kBoundMax);
        if (BNB && v == x.obj_var) {
          // XLessY(var, Constant(best)) / x_greater_y(var, Constant(best)) on their first run (x_less_y.rs:104-109 against term/constant.rs:49-52);
          // "no solution yet" is +-(PCP_BOUND_MAX + 1): then nothing moves.  A fold that would empty the cell is not applied (bnb_fold_kernel's rule)
          if (x.obj_mode == PCP_MINIMIZE) {
            if (best - 1 < u) { if (best - 1 < l) fold_empty = true; else u = best - 1; }
          } else if (best + 1 > l) {
            if (best + 1 > u) fold_empty = true; else l = best + 1;
          }
        }
      } else if (v - V >= a.m.sums.count) {
        l = u = a.m.const_val[v - V];  // (the Sum slots in between hold nothing: their domain is computed from the members)
      }
      dom[v] = make_int2(-l, u);
    }
    if (__ballot(wide)) {  // a bound beyond +-(2^29 - 1): refused, not wrapped (pcp_hip.h)
      if (lane == 0) { a.status[node] = kStatusRetry; atomicMax(a.violation, 1u); if (BNB) x.empty[node] = 0; }
      continue;
    }
    if (BNB) {
      const bool emptied = __ballot(fold_empty) != 0;
      if (lane == 0) x.empty[node] = emptied ? 1 : 0;
      if (emptied) {  // the bound alone fails the node: PCP_FALSE, the row as it went in
        if (a.lb_out != a.lb_in)
          for (uint32_t v = lane; v < V; v += 64) a.lb_out[row + v] = a.lb_in[row + v];
        if (a.ub_out != a.ub_in)
          for (uint32_t v = lane; v < V; v += 64) a.ub_out[row + v] = a.ub_in[row + v];
        wave_sync();
        if (a.active_out)  // (a failed node keeps the units it came with)
          for (uint32_t w = lane; w < words64; w += 64) {
            const uint64_t lo = live[2 * w], hi = (2 * w + 1 < Wu) ? live[2 * w + 1] : 0u;
            a.active_out[(size_t)node * words64 + w] = lo | (hi << 32);
          }
        if (lane == 0) a.status[node] = (uint8_t)PCP_FALSE;
        acc_waves += 1; acc_nodes += 1; acc_failed += 1;
        wave_sync();
        continue;
      }
    }
    if (__ballot(bad) && lane == 0) misc[F_FAIL] = 1u;
    wave_sync();

    // ---- rounds: the node's exclusions, then every live unit, once per round, until a round narrows nothing -----------------------------------
    Ctr ctr;
    const LdsDom dm{dom, 1u, chg, &misc[F_FAIL], 1u, &ctr, a.m.sums};
    uint32_t steps2 = 0, steps3 = 0, rounds = 0;
    bool failed = __builtin_amdgcn_readfirstlane(misc[F_FAIL]) != 0;
    const uint32_t e0 = x.excl_off ? x.excl_off[node] : 0u, e1 = x.excl_off ? x.excl_off[node + 1] : 0u;
    bool ex_open = false;  // one of the exclusions is not entailed
    while (!failed) {
      ++rounds;
      const uint32_t before = ctr.narrow;
      ex_open = false;
      for (uint32_t i = e0 + lane; i < e1; i += 64) {
        const pcp_excl e = x.excl[i];
        if (e.var >= V) { dm.set_fail(); misc[F_OOB] = 1u; continue; }  // malformed: the node is refused
        const int K = e.value;
        const int2 c_ = dom[e.var];
        const int xl0 = -c_.x, xu0 = c_.y;
        int xl = xl0, xu = xu0;
        ++steps2;
        // XNeqY(Identity(var), Constant(value))::propagate (x_neq_y.rs:82-93): a value is removed only at a bound
        if (xl0 == xu0) { if (xl0 == K) { dm.set_fail(); continue; } }
        else if (K == xl0) xl = xl0 + 1;
        else if (K == xu0) xu = xu0 - 1;
        if (xl > xl0) dm.raise_lb(e.var, xl);
        if (xu < xu0) dm.lower_ub(e.var, xu);
        ex_open |= !(K < xl || K > xu);  // is_subsumed() on what propagate() left (store.rs:166-175): True iff disjoint (x_neq_y.rs:71-73)
      }
      wave_sync();
      for (uint32_t u = lane; u < U; u += 64) {
        if (!((live[u >> 5] >> (u & 31u)) & 1u)) continue;
        const bool entailed = form_unit_step(a.nodes, a.unit_root, a.m.recs, u, dm, steps2, steps3);
        if (entailed) atomicAnd(&live[u >> 5], ~(1u << (u & 31u)));      // unlink_prop (store.rs:200-207)
      }
      wave_sync();
      failed = __builtin_amdgcn_readfirstlane(misc[F_FAIL]) != 0;
      if (!__ballot(ctr.narrow != before)) break;
    }

    if (__builtin_amdgcn_readfirstlane(misc[F_OOB]) != 0) {  // an entry with var >= n_vars: the node is refused, its outputs left alone
      if (lane == 0) { a.status[node] = kStatusRetry; atomicMax(a.violation, 1u); }
      wave_sync();
      continue;
    }
    // ---- write back, status (store.rs:250-256) ------------------------------------------------------------------------------------------------
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
    const bool unknown = __ballot(any_live || ex_open) != 0;
    if (lane == 0) a.status[node] = failed ? (uint8_t)PCP_FALSE : (unknown ? (uint8_t)PCP_UNKNOWN : (uint8_t)PCP_TRUE);
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

hipError_t launch_formexcl(const FormExclArgs& x, const LaunchPlan& p, hipStream_t stream) {
  if (!x.f.m.recs || !x.f.nodes || !x.f.unit_root || !x.f.status || (x.excl_off && !x.excl)) return hipErrorInvalidValue;
  const bool bnb = x.obj_best != nullptr;
  if (bnb && !x.empty) return hipErrorInvalidValue;
  const void* fn = bnb ? reinterpret_cast<const void*>(formexcl_kernel<true>) : reinterpret_cast<const void*>(formexcl_kernel<false>);
  if (p.lds_bytes > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes);
    if (e != hipSuccess) return e;
  }
  if (bnb) hipLaunchKernelGGL(formexcl_kernel<true>, dim3(p.grid), dim3(p.block), p.lds_bytes, stream, x);
  else hipLaunchKernelGGL(formexcl_kernel<false>, dim3(p.grid), dim3(p.block), p.lds_bytes, stream, x);
  return hipGetLastError();
}

}  // namespace pcp
