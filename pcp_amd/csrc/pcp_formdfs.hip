// pcp_formdfs.hip — the search loop over Interval<i32> stores that hold FORMULA propagators, on the device: what pcp_dfs_device does for such
// a store with three launches per node (formfix_kernel on the top row, then dfs_step_kernel), for MANY trees inside one launch.  gfx950.
//
// ≡ OneSolution / AllSolution<Propagation<Brancher<FirstSmallestVar, MiddleVal, BinarySplit>>> over a VectorStack (search/mod.rs:45-52,
// search/engine/one_solution.rs:92-105) under Monitor<Statistics, StopNode> (search/monitor.rs:19-68, search/stop_node.rs:47-62), and with
// BNB = true BranchAndBound around it (search/branch_and_bound.rs:64-84).  This is the forest the scheduling models live in:
// propagators::Cumulative::join (propagators/cumulative.rs:59-114) allocates equivalences over Boolean, XEqYMulZ and Sum views, which set
// mode refuses.
//
// MI355X mapping: a formula store is small — a node is a few hundred bytes of LDS — so a tree is ONE WAVEFRONT, up to four trees per
// 256-thread workgroup, each on its own LDS slice (form_carve, the slice of formfix_kernel: nothing more is needed, the loop's own state is
// wave-uniform and sits in registers).  A tree is a latency chain; a CU wants as many chains as its registers allow.
// There is no workgroup barrier: the trees of a workgroup never wait for each other.
//
// Tree t works on slice t of a pcp_dfs_state laid out as for pcp_dfs_forest_device: a stack of (lb, ub) rows in HBM, rows [0, sp) open.  What
// a caller sees between two launches — sp, those rows, the counters, stop — is what pcp_dfs_device leaves after the same number of steps
// (dfs_step_kernel, pcp_kernels.hip, is the specification), so the host loop moves bottom rows between stacks and ranks as it does for the
// all-XNeqY forest.  Inside a launch:
//   - the left child is never read back: after the branch it IS the LDS node, with ub[var] lowered; its row is written only when the launch
//     ends with it on top of the stack;
//   - unit liveness is derived, never stored: an entailed unit stays entailed as domains shrink, so the descent to the left
//     child keeps the live bits; popping any other row sets every unit live, and the first round unlinks again what is entailed.
#include <algorithm>

#include "pcp_formula.hpp"

namespace pcp {

namespace {

// SINK = true (never with BNB): every solution is appended to the context's solution sink (SinkDev, pcp_neq.h) as a whole (lb, ub) row — a
// True node is a box, not a point.  A template flag, so that the instantiations without a sink are the code they were.
template <bool BNB, bool SINK>
__global__ void __launch_bounds__(256) formdfs_kernel(const FormDfsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nwv = blockDim.x >> 6;
  const uint32_t t = blockIdx.x * nwv + wv;
  if (t >= a.n_trees) return;  // (wave-uniform: the other trees of the workgroup never wait for this one)
  uint32_t sp = a.sp[t], stop = a.stop[t];
  if (sp == 0 || stop) return;
  if (sp > a.capacity) {  // (a stack pointer beyond the rows the caller gave: no row is touched)
    if (lane == 0) { a.counters[(size_t)t * 5 + 3] = 1; a.stop[t] = 1u; }
    return;
  }
  const uint32_t V = a.m.n_vars, S = a.m.n_slots, Wv = (S + 31) >> 5, U = a.n_units, Wu = (U + 31) >> 5;
  const FormCarve cv = form_carve(S, U);
  unsigned char* const mine = smem + (size_t)wv * cv.total;
  int2* const dom = reinterpret_cast<int2*>(mine + cv.dom);
  uint32_t* const chg = reinterpret_cast<uint32_t*>(mine + cv.chg);
  uint32_t* const live = reinterpret_cast<uint32_t*>(mine + cv.live);
  uint32_t* const misc = reinterpret_cast<uint32_t*>(mine + cv.misc);
  auto wave_sync = [] { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier(); };
  int32_t* const lb = a.lb + (size_t)t * a.capacity * V;
  int32_t* const ub = a.ub + (size_t)t * a.capacity * V;
  unsigned long long* const cnt = a.counters + (size_t)t * 5;
  unsigned long long nodes = cnt[0];
  const bool want_first = !BNB && a.first_solution != nullptr && cnt[1] == 0;  // the forest keeps each tree's FIRST solution
  uint32_t n_sol = 0, n_failed = 0, error = 0, wrote_first = 0;
  uint32_t steps2 = 0, steps3 = 0, acc_rounds = 0, acc_nodes = 0;  // (per lane resp. uniform; reduced and flushed once)
  Ctr ctr;
  const LdsDom dm{dom, 1u, chg, &misc[F_FAIL], 1u, &ctr, a.m.sums};

  if (lane < (uint32_t)F_WORDS) misc[lane] = 0;
  for (uint32_t w = lane; w < Wv; w += 64) chg[w] = 0;
  // The constants' cells (the Sum slots in between hold nothing: their domain is computed from the members).  Only a node that FAILS can
  // have narrowed one (Constant::update, term/constant.rs:49-52: a narrowed constant is an empty one), so they are written again after a
  // failed node only
  auto store_consts = [&] {
    for (uint32_t v = V + lane; v < S; v += 64) {
      const int c = (v - V >= a.m.sums.count) ? a.m.const_val[v - V] : 0;
      dom[v] = make_int2(-c, c);
    }
  };
  store_consts();
  // the node in LDS: its lower bounds (a solution's row)
  auto store_lbs = [&](int32_t* out) { for (uint32_t v = lane; v < V; v += 64) out[v] = -dom[v].x; };
  // ... and the whole node, as row r of the stack
  auto store_row = [&](uint32_t r) {
    for (uint32_t v = lane; v < V; v += 64) { const int2 d = dom[v]; lb[(size_t)r * V + v] = -d.x; ub[(size_t)r * V + v] = d.y; }
  };

  bool in_lds = false;  // the row on top of the stack is the LDS node (the left child of the node before) and has not been written
  for (uint32_t step = 0; step < a.n_steps && sp != 0 && !stop; ++step) {
    // ---- pop: row sp - 1 as (-lb, ub) cells ---------------------------------------------------------------------------------------------
    const uint32_t node = sp - 1;
    bool bad = false;
    if (lane == 0) misc[F_FAIL] = 0;
    if (!in_lds) {
      bool wide = false;
      for (uint32_t v = lane; v < V; v += 64) {
        const int l = lb[(size_t)node * V + v], u = ub[(size_t)node * V + v];
        bad |= l > u;
        wide |= (l < -kBoundMax) | (l > kBoundMax) | (u < -kBoundMax) | (u > kBoundMax);
        dom[v] = make_int2(-l, u);
      }
      for (uint32_t w = lane; w < Wu; w += 64) live[w] = (w == Wu - 1 && (U & 31u)) ? (1u << (U & 31u)) - 1u : 0xFFFFFFFFu;
      if (__ballot(wide)) {
        // a bound beyond +-(2^29 - 1): refused, not wrapped (pcp_hip.h).  dfs_step_kernel counts the refused node, pops it and stops: error 2
        if (lane == 0) atomicMax(a.violation, 1u);
        ++nodes; error = 2; stop = 1; sp = node;
        break;
      }
    }
    in_lds = false;
    wave_sync();
    if (BNB) {
      // the bound propagator of BranchAndBound, folded (branch_and_bound.rs:64-84): var < best resp. var > best on the incumbent as it is
      // NOW.  "No solution yet" (+-(PCP_BOUND_MAX + 1)) narrows nothing.  The fold stays in the node: the right child inherits it and
      // folds again when it is popped (search._IntervalRows.propagate)
      const long long best = __hip_atomic_load(a.obj_best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      int2 d = dom[a.obj_var];
      const long long lim = (long long)kBoundMax + 1;
      if (a.obj_mode == PCP_MINIMIZE) d.y = (int)min((long long)d.y, max(best - 1, -lim));
      else d.x = (int)min((long long)d.x, -min(best + 1, lim));
      bad |= -d.x > d.y;  // a node the fold empties is a node and a failed node, and no unit runs
      if (lane == 0) dom[a.obj_var] = d;
      wave_sync();
    }

    // ---- propagate: Jacobi rounds over the live units until a round narrows nothing or the node fails ------------------------------------
    bool failed = __ballot(bad) != 0;
    uint32_t rounds = 0;
    while (!failed) {
      ++rounds;
      const uint32_t before = ctr.narrow;
      for (uint32_t u = lane; u < U; u += 64) {
        if (!((live[u >> 5] >> (u & 31u)) & 1u)) continue;
        if (form_unit_step(a.nodes, a.unit_root, a.m.recs, u, dm, steps2, steps3))
          atomicAnd(&live[u >> 5], ~(1u << (u & 31u)));  // unlink_prop (store.rs:200-207)
      }
      wave_sync();
      failed = __builtin_amdgcn_readfirstlane(misc[F_FAIL]) != 0;
      if (!__ballot(ctr.narrow != before)) break;
    }
    acc_rounds += rounds ? rounds : 1;
    ++acc_nodes;

    // ---- Consistency::consistency (store.rs:250-256): False if a propagate failed, True if no subscription remains, else Unknown; and the
    //      key of FirstSmallestVar (first_smallest_var.rs:30-39): the smallest size > 1, the lowest index on a tie -------------------------
    bool emptied = false, any_live = false;
    unsigned long long key = ~0ull;
    for (uint32_t v = lane; v < V; v += 64) {
      const int2 d = dom[v];
      emptied |= -d.x > d.y;
      const unsigned long long size = (unsigned long long)((long long)d.y + (long long)d.x + 1);
      if (size > 1) key = min(key, (size << 32) | v);
    }
    for (uint32_t w = lane; w < Wu; w += 64) any_live |= live[w] != 0;
    failed = failed || __ballot(emptied) != 0;
    const bool unknown = !failed && __ballot(any_live) != 0;

    // ---- the step of dfs_step_kernel ----------------------------------------------------------------------------------------------------
    uint32_t new_sp = sp - 1;
    if (unknown) {
      for (int o = 32; o > 0; o >>= 1) key = min(key, (unsigned long long)__shfl_xor(key, o));
      if (key == ~0ull || sp >= a.capacity) {
        // 1: the stack is full — the node stays on the stack, propagated and uncounted: a caller that resumes with a larger stack runs it
        // again (idempotent) and counts it then.  3: Unknown, yet no variable with more than one value: the reference panics here
        // (first_smallest_var.rs:36)
        store_row(node);
        error = key == ~0ull ? 3u : 1u; stop = 1;
        break;
      }
      const uint32_t var = (uint32_t)key;
      const int2 dv = dom[var];
      const int val = (int)(((long long)dv.y - (long long)dv.x) / 2);  // MiddleVal (middle_val.rs:25-27): `/` truncates toward zero like Rust's
      // Brancher (brancher.rs:52-71, binary_split.rs:46-57): the parent's row becomes the right child `x > val`; the left child `x <= val`
      // goes on top — it is the LDS node from here on
      for (uint32_t v = lane; v < V; v += 64) {
        const int2 d = dom[v];
        lb[(size_t)node * V + v] = (v == var) ? max(-d.x, val + 1) : -d.x;
        ub[(size_t)node * V + v] = d.y;
        if (v == var) dom[v].y = min(d.y, val);
      }
      new_sp = sp + 1;
      in_lds = true;
    }
    if constexpr (SINK) {
      // A solution draws its ticket BEFORE it is counted (the limit node, `nodes + 1` at the limit, is no solution and draws none).  6: the
      // sink is full — the node stays on the stack, propagated and uncounted, and a caller that drains the sink and resumes runs it again
      // (idempotent), counts it then and appends it then (the contract of error 1)
      if (!failed && !unknown && !(a.node_limit && nodes + 1 >= a.node_limit)) {
        uint32_t slot = 0;
        if (lane == 0) slot = __hip_atomic_fetch_add(a.sink.count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        slot = __builtin_amdgcn_readfirstlane(slot);
        if (slot >= a.sink.capacity) {
          store_row(node);
          error = kDfsSinkFull; stop = 1;
          break;
        }
        for (uint32_t v = lane; v < V; v += 64) { const int2 d = dom[v]; a.sink.lb[(size_t)slot * V + v] = -d.x; a.sink.ub[(size_t)slot * V + v] = d.y; }
        if (lane == 0 && a.sink.tree) a.sink.tree[slot] = t;
      }
    }
    // Monitor<Statistics, StopNode>: the node that reaches the limit is a node, but neither a solution nor a failure (stop_node.rs:57-62, 90-97)
    ++nodes;
    const bool last = a.node_limit && nodes >= a.node_limit;
    if (!failed && !unknown && !last) {
      ++n_sol;
      if (BNB) {
        // the incumbent becomes var.lower() in both modes; within a tree every solution beats the one before
        const int value = -dom[a.obj_var].x;
        if (a.tree_row) store_lbs(a.tree_row + (size_t)t * V);
        if (lane == 0) {
          a.tree_best[t] = value;
          if (a.obj_mode == PCP_MINIMIZE) atomicMin(a.obj_best, value); else atomicMax(a.obj_best, value);
        }
      } else {
        if (want_first && !wrote_first) { store_lbs(a.first_solution + (size_t)t * V); wrote_first = 1; }
        if (a.stop_on_solution) stop = 1;
      }
    } else if (failed && !last) {
      ++n_failed;
    }
    if (failed) store_consts();
    if (last) stop = 1;
    sp = new_sp;
    wave_sync();  // (the branch's LDS write, and this tree's rows, before the next pop reads them)
  }

  if (in_lds) store_row(sp - 1);  // the left child nobody has popped yet
  for (int o = 32; o > 0; o >>= 1) { steps2 += __shfl_down(steps2, o); steps3 += __shfl_down(steps3, o); ctr.narrow += __shfl_down(ctr.narrow, o); }
  if (lane == 0) {
    a.sp[t] = sp; a.stop[t] = stop;
    cnt[0] = nodes;
    if (n_sol) cnt[1] += n_sol;
    if (n_failed) cnt[2] += n_failed;
    if (error) cnt[3] = error;
    if (wrote_first) cnt[4] = 2;  // (dfs_step_kernel's flag: the first solution has been copied)
    pcp_stats* const stats = a.stats + (blockIdx.x & (kStatSlots - 1));
    const unsigned long long ev = (unsigned long long)steps2 + steps3;
    if (steps2) atomicAdd((unsigned long long*)&stats->steps, (unsigned long long)steps2);
    if (steps3) atomicAdd((unsigned long long*)&stats->steps3, (unsigned long long)steps3);
    if (ev) { atomicAdd((unsigned long long*)&stats->evaluated, ev); atomicAdd((unsigned long long*)&stats->full_evals, ev); }
    if (ctr.narrow) atomicAdd((unsigned long long*)&stats->narrowings, (unsigned long long)ctr.narrow);
    if (acc_rounds) atomicAdd((unsigned long long*)&stats->waves, (unsigned long long)acc_rounds);
    if (acc_nodes) atomicAdd((unsigned long long*)&stats->nodes, (unsigned long long)acc_nodes);
    if (n_failed) atomicAdd((unsigned long long*)&stats->failed_nodes, (unsigned long long)n_failed);
  }
}

template <bool BNB, bool SINK>
hipError_t launch_formdfs_as(const FormDfsArgs& a, const LaunchPlan& p, hipStream_t stream) {
  hipError_t e;
  if (p.lds_bytes > 64 * 1024 &&
      (e = hipFuncSetAttribute(reinterpret_cast<const void*>(formdfs_kernel<BNB, SINK>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes)) != hipSuccess)
    return e;
  hipLaunchKernelGGL((formdfs_kernel<BNB, SINK>), dim3(p.grid), dim3(p.block), p.lds_bytes, stream, a);
  return hipGetLastError();
}

}  // namespace

size_t lds_bytes_formdfs(uint32_t n_slots, uint32_t n_units, uint32_t waves) {
  const FormCarve c = form_carve(n_slots, n_units);
  return c.total * waves <= 160 * 1024 ? c.total * waves : 0;
}

// p.block = 64 x the trees of a workgroup, p.grid = ceil(n_trees / those), p.lds_bytes = lds_bytes_formdfs of them
hipError_t launch_formdfs(const FormDfsArgs& a, bool bnb, const LaunchPlan& p, hipStream_t stream) {
  if (a.sink.lb) {  // the context's solution sink (pcp_solution_sink_set); the branch-and-bound entries refuse it
    if (bnb || !a.sink.ub || !a.sink.count || !a.sink.capacity) return hipErrorInvalidValue;
    return launch_formdfs_as<false, true>(a, p, stream);
  }
  return bnb ? launch_formdfs_as<true, false>(a, p, stream) : launch_formdfs_as<false, false>(a, p, stream);
}

}  // namespace pcp
