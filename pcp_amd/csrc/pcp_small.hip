// pcp_small.hip — the propagation fixpoint of SMALL stores (gfx950): a few dozen variables, up to a few thousand elementary filters — BASELINE
// config 4 (the Golomb-ruler network: 55 variables, one Distinct of 990 XNeqY, 45 XEqYPlusZ, 10 XLessY / XEqY), the reference's own test models.
//
// Same contract as fixpoint_kernel (pcp_kernels.hip): Store::consistency = prepare() + propagation_loop() (propagation/store.rs:125-164,
// 247-257) for a batch of nodes, explicit unit-level `active` rows or implicit-active nodes: every active propagator once
// (init_scheduler, store.rs:144-149), then again while anything changes (Store::react wakes the propagators of a changed variable,
// store.rs:191-198; on a store this small "all of them" is cheaper than finding out which); an entailed unit is unlinked (store.rs:200-207).
//
// MI355X mapping: ONE WAVEFRONT PER NODE.  The generic kernel gives a tile of 16 such nodes a 1024-thread workgroup and runs the machinery
// it needs for million-record models (packed tiles, bulk range tests, changed-pair lists, workgroup barriers between rounds): 0.70 ms for 4096
// nodes of 440 bytes, none of it spent on filters.  Here a node's domains are an LDS slice of its wavefront ((-lb, ub) cells: both narrowings
// are ds_min), the records come from an LDS copy the workgroup shares, a round is every live record once, lane-strided, and rounds are
// separated by a wavefront barrier only; sixteen wavefronts per CU run sixteen nodes at sixteen different points of their fixpoints.  A round's
// last pass — the one that narrows nothing — has evaluated every live record on the final domains, so its is_subsumed() results ARE the units'
// entailment: a unit all of whose members are entailed is unlinked.
// ALL-DIFFERENT units (Distinct::new, propagators/distinct.rs:63-83: x != y over every pair of a variable set; the host recognises them)
// are filtered as a group, lane = variable: the assigned variables' values go into a 128-bit mask above the unit's smallest lower bound
// (an LDS atomicOr: a bit that was already set is two variables with one value — the node fails, as the pair's filter would make it);
// every other variable moves its bounds past the values in the mask.  Pair by pair the reference removes a value only at a bound and only
// against an assigned partner (x_neq_y.rs:82-93), one value per wake-up: the mask does the same removals, all at once — same fixpoint
// ("jump windows").  990 pair filters of config 4's Distinct become one step of 45 lanes.  A unit whose values span more than
// 128 falls back to its pairs for that round.  Integer bound work: no MFMA.
#include <algorithm>

#include "pcp_small.hpp"  // the LDS carve, the copy of the records and the round, shared with pcp_smalldfs.hip

namespace pcp {

__global__ void __launch_bounds__(256) smallfix_kernel(const SmallArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6), nwv = blockDim.x >> 6;
  const uint32_t V = a.m.n_vars, S = a.m.n_slots, P = a.m.n_recs, U = a.n_units, Wu = (U + 31) >> 5, Wv = (S + 31) >> 5, words64 = (U + 63) >> 6;
  // the workgroup's copy of the records, then one slice per wavefront: cells, a (dummy) changed mask, the live units, the entailed units, flags
  const SmallShared sh = small_copy_shared(smem, P, a.m.recs, a.rec_unit, a.ad_tab, a.ad_vars);
  const SmallSlice sl = small_slice(smem, P, S, U, wv);
  int2* const dom = sl.dom;
  uint32_t* const chg = sl.chg;
  uint32_t* const live = sl.live;
  uint32_t* const ent = sl.ent;
  uint32_t* const misc = sl.misc;
  __syncthreads();
  auto wave_sync = [] { small_wave_sync(); };
  pcp_stats* const stats = a.stats + (blockIdx.x & (kStatSlots - 1));
  unsigned long long acc_s2 = 0, acc_s3 = 0, acc_narrow = 0, acc_waves = 0, acc_nodes = 0, acc_failed = 0;

  uint32_t first = blockIdx.x * nwv + wv, stride = gridDim.x * nwv, n_nodes = a.n_nodes;
  size_t row_base = 0;
  uint32_t st_base = 0;
  if (a.sp_ptr) {  // host-stepped device-side DFS (pcp_dfs_device): ONE node, the one on top of the stack
    const uint32_t sp = *a.sp_ptr;
    if (sp == 0 || *a.stop_ptr) return;
    row_base = (size_t)(sp - 1) * V; st_base = sp - 1; n_nodes = 1;
  }
  for (uint32_t node = first; node < n_nodes; node += stride) {
    const size_t row = row_base + (size_t)node * V;
    // ---- stage: the node's domains, its live units -----------------------------------------------------------------------------------------
    if (lane < (uint32_t)S_WORDS) misc[lane] = 0;
    for (uint32_t w = lane; w < Wv; w += 64) chg[w] = 0;
    for (uint32_t w = lane; w < Wu; w += 64) {  // Store::active (one bit per unit): the caller's row, or every unit (implicit-active nodes)
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
    if (__ballot(bad) && lane == 0) misc[S_FAIL] = 1u;
    wave_sync();

    // ---- rounds: every record of a live unit once per round, until a round narrows nothing ------------------------------------------------
    Ctr ctr;
    const LdsDom dm{dom, 1u, chg, &misc[S_FAIL], 1u, &ctr, a.m.sums};
    uint32_t s2 = 0, s3 = 0, rounds = 0;
    bool failed = __builtin_amdgcn_readfirstlane(misc[S_FAIL]) != 0;
    // the node's OWN propagators (pcp_propagate_device_units): what a branch appends to ONE node's cstore and what cannot be folded into its
    // bounds — Enumerate's  x != v  with v inside the domain (search/branching/enumerate.rs:48-59; it stays active until v reaches a bound).
    // One variable against one Constant, kinds XNeqY / XEqY / XLessY; lane-strided like the records; `nu_open`: one of them is not entailed.
    const uint32_t nu0 = a.nu_off ? a.nu_off[node] : 0u, nu1 = a.nu_off ? a.nu_off[node + 1] : 0u;
    bool nu_open = false;
    while (!failed) {
      ++rounds;
      const uint32_t before = ctr.narrow;
      nu_open = false;
      small_round(sh, P, Wu, sl, dm, lane, s2, s3, [&] {
        for (uint32_t i = nu0 + lane; i < nu1; i += 64) {
          const pcp_prop p = a.nu[i];
          // x + ox (kind) c  <=>  x (kind) K = c - ox;   c (kind) y + oy  <=>  y != K | y = K | y > K  with K = c - oy   (term/addition.rs:98, cmp/mod.rs:40-60)
          const bool cy = p.var[1] == PCP_CONST, cx = p.var[0] == PCP_CONST;
          const uint32_t v = cy ? p.var[0] : p.var[1];
          if (cx == cy || v >= V || p.kind > PCP_LT) { dm.set_fail(); misc[S_OOB] = 1u; continue; }  // malformed: the node is refused
          const long long K64 = cy ? (long long)p.off[1] - p.off[0] : (long long)p.off[0] - p.off[1];
          const int K = (int)max(-(long long)kBoundMax - 2, min((long long)kBoundMax + 2, K64));  // (beyond every bound either way)
          const uint32_t op = p.kind == PCP_NEQ ? 3u : p.kind == PCP_EQ ? 2u : (cy ? 0u : 1u);  // 0 "< K", 1 "> K", 2 "= K", 3 "!= K"
          const int2 c_ = dom[v];
          const int xl0 = -c_.x, xu0 = c_.y;
          int xl = xl0, xu = xu0;
          ++s2;
          if (op == 0u) xu = min(xu0, K - 1);           // XLessY::propagate (x_less_y.rs:104-109) against Constant::update (term/constant.rs:49-52)
          else if (op == 1u) xl = max(xl0, K + 1);
          else if (op == 2u) { xl = max(xl0, K); xu = min(xu0, K); }  // XEqY (x_eq_y.rs:102-107)
          else {                                        // XNeqY (x_neq_y.rs:82-93): a value is removed only at a bound
            if (xl0 == xu0 && xl0 == K) { dm.set_fail(); continue; }
            if (xl0 != xu0) { if (K == xl0) xl = xl0 + 1; else if (K == xu0) xu = xu0 - 1; }
          }
          if (xl > xu) { dm.set_fail(); continue; }
          if (xl > xl0) dm.raise_lb(v, xl);
          if (xu < xu0) dm.lower_ub(v, xu);
          // is_subsumed() on what propagate() left (store.rs:166-175)
          const bool entailed = op == 0u ? xu < K : op == 1u ? xl > K : op == 2u ? (xl == K && xu == K) : (K < xl || K > xu);
          nu_open |= !entailed;
        }
      });
      wave_sync();
      failed = __builtin_amdgcn_readfirstlane(misc[S_FAIL]) != 0;
      if (!__ballot(ctr.narrow != before)) break;
    }

    if (__builtin_amdgcn_readfirstlane(misc[S_OOB]) != 0) {  // a malformed node unit: the node is refused, its outputs left alone
      if (lane == 0) { a.status[st_base + node] = kStatusRetry; atomicMax(a.violation, 1u); }
      wave_sync();
      continue;
    }
    // ---- write back, unlink the entailed units (store.rs:200-207), status (store.rs:250-256) --------------------------------------------------
    bool emptied = false;
    for (uint32_t v = lane; v < V; v += 64) {
      const int2 d = dom[v];
      emptied |= -d.x > d.y;
      a.lb_out[row + v] = -d.x; a.ub_out[row + v] = d.y;
    }
    failed = failed || __ballot(emptied) != 0;
    bool any_live = false;
    for (uint32_t w = lane; w < Wu; w += 64) {
      const uint32_t left = failed ? live[w] : live[w] & ~ent[w];
      live[w] = left;
      any_live |= left != 0;
    }
    wave_sync();
    if (a.active_out)
      for (uint32_t w = lane; w < words64; w += 64) {
        const uint64_t lo = live[2 * w], hi = (2 * w + 1 < Wu) ? live[2 * w + 1] : 0u;
        a.active_out[(size_t)node * words64 + w] = lo | (hi << 32);
      }
    const bool unknown = __ballot(any_live || nu_open) != 0;
    if (lane == 0) a.status[st_base + node] = failed ? (uint8_t)PCP_FALSE : (unknown ? (uint8_t)PCP_UNKNOWN : (uint8_t)PCP_TRUE);
    for (int o = 32; o > 0; o >>= 1) { s2 += __shfl_down(s2, o); s3 += __shfl_down(s3, o); ctr.narrow += __shfl_down(ctr.narrow, o); }
    acc_s2 += s2; acc_s3 += s3; acc_narrow += ctr.narrow; acc_waves += rounds ? rounds : 1; acc_nodes += 1; acc_failed += failed ? 1 : 0;
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
    if (a.dbg && acc_nodes) atomicAdd(&a.dbg[(size_t)(blockIdx.x & (kStatSlots - 1)) * PCP_DBG_COUNT + PCP_DBG_SMALL_NODES], acc_nodes);
  }
}

size_t lds_bytes_small(uint32_t n_slots, uint32_t n_units, uint32_t n_recs, uint32_t waves) {
  const size_t b = small_shared_bytes(n_recs) + (size_t)waves * small_wave_bytes(n_slots, n_units);
  return b <= 160 * 1024 ? b : 0;
}

hipError_t launch_smallfix(const SmallArgs& a, const LaunchPlan& p, hipStream_t stream) {
  if (!a.m.recs || !a.status) return hipErrorInvalidValue;
  if (p.lds_bytes > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(smallfix_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(smallfix_kernel, dim3(p.grid), dim3(p.block), p.lds_bytes, stream, a);
  return hipGetLastError();
}

}  // namespace pcp