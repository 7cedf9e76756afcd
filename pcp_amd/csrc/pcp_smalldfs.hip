// pcp_smalldfs.hip — the search loop over SMALL Interval<i32> stores of plain propagators, on the device: what pcp_dfs_device does for such a
// store with three launches per node (a fixpoint kernel on the top row, then dfs_step_kernel), for MANY trees inside one launch.  gfx950.
// These are the stores smallfix_kernel propagates (pcp_small.hip, plan.path 4): at most 128 slots and 2048 elementary filters, no formula
// units — Distinct, XLessY, XEqY, XEqYPlusZ, XLessYPlusZ, XGreaterYPlusZ, XEqYMulZ and Sum views in any mixture; BASELINE config 4, the
// Golomb-ruler network, is one of them, and the only optimisation benchmark of the project.
//
// ≡ OneSolution / AllSolution<Propagation<Brancher<FirstSmallestVar, MiddleVal, BinarySplit>>> over a VectorStack (search/mod.rs:45-52,
// search/engine/one_solution.rs:92-105) under Monitor<Statistics, StopNode> (search/monitor.rs:19-68, search/stop_node.rs:47-62), and with
// BNB = true BranchAndBound around it (search/branch_and_bound.rs:64-84).
//
// MI355X mapping: the loop of formdfs_kernel (pcp_formdfs.hip) — a tree is ONE WAVEFRONT, up to four trees per 256-thread workgroup, each
// on its own LDS slice, the loop's own state wave-uniform in registers — with smallfix_kernel's round as the propagation step
// (pcp_small.hpp: the all-different units through their 128-value mask, then every record of a live unit, lane-strided).  The records
// come from ONE LDS copy per workgroup, made once per launch by all its wavefronts and published by the kernel's only __syncthreads();
// every wavefront reaches that barrier — a workgroup with three trees, or with a finished one, leaves nobody behind it — and only then
// takes its wave-uniform exits.  After it the trees of a workgroup never wait for each other.
//
// Tree t works on slice t of a pcp_dfs_state laid out as for pcp_dfs_forest_device: a stack of (lb, ub) rows in HBM, rows [0, sp) open.  What
// a caller sees between two launches — sp, those rows, the counters, stop — is what pcp_dfs_device leaves after the same number of steps
// (dfs_step_kernel, pcp_kernels.hip, is the specification), so the host loop moves bottom rows between stacks and ranks as it does for the
// other interval forests.  Inside a launch:
//   - the left child is never read back: after the branch it IS the LDS node, with ub[var] lowered; its row is written only when the launch
//     ends with it on top of the stack;
//   - unit liveness is derived, never stored: an entailed unit stays entailed as domains shrink, so the descent to the left
//     child keeps the live bits; popping any other row sets every unit live, and the round that narrows nothing unlinks again what is
//     entailed (`ent`, as in smallfix_kernel).
//
// ENUM = true: the same loop under Brancher<FirstSmallestVar, MiddleVal | MinVal, Enumerate> (search/branching/enumerate.rs:33-60):
// pcp_dfs_forest_device_small_enum.  The children are `x = v` and `x != v`; an interior `x != v` removes nothing from an Interval and stays
// with its node as a pcp_excl entry (pcp_smallexcl.hip).  The batched search carries a CSR list per open node and copies it at every
// branch; a depth-first tree needs none of that: every open row of the stack is the right child of an ancestor of the current node, so its
// list is a PREFIX of the exclusions appended along the current path plus at most one entry of its own.  A tree keeps ONE path of
// entries in HBM and per stack row (row_base, row_excl) — how many path entries the row inherits and the entry appended when it is popped.
// The current node's list is path[0 .. n), n wave-uniform in a register and re-derived from the top row at every launch; nothing is
// copied at a branch.  Entries are never filtered out of the path: an entry whose value lies outside [lb, ub] is entailed and stays so
// (domains only shrink below a node), and the value rule only looks inside [lb, ub] — the same tree as search.branch_enumerate's lists.
// Integer bound work: no MFMA.
#include <algorithm>

#include "pcp_small.hpp"

namespace pcp {

namespace {

constexpr uint32_t kNoExcl = 0xFFFFFFFFu;  // row_excl[r].var: the row appends nothing when it is popped

// SINK = true (never with BNB): every solution is appended to the context's solution sink (SinkDev, pcp_neq.h) as a whole (lb, ub) row — a
// True node is a box, not a point.  A template flag, so that the instantiations without a sink are the code they were.
template <bool BNB, bool ENUM, bool SINK>
__global__ void __launch_bounds__(256) smalldfs_kernel(const SmallDfsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nwv = blockDim.x >> 6;
  const uint32_t V = a.m.n_vars, S = a.m.n_slots, P = a.m.n_recs, Wv = (S + 31) >> 5, U = a.n_units, Wu = (U + 31) >> 5;
  // the records, once per launch, by every wavefront of the workgroup — also those that have no tree to run
  const SmallShared sh = small_copy_shared(smem, P, a.m.recs, a.rec_unit, a.ad_tab, a.ad_vars);
  __syncthreads();
  const uint32_t t = blockIdx.x * nwv + wv;
  if (t >= a.n_trees) return;  // (wave-uniform, and behind the barrier: the other trees of the workgroup never wait for this one)
  uint32_t sp = a.sp[t], stop = a.stop[t];
  if (sp == 0 || stop) return;
  if (sp > a.capacity) {  // (a stack pointer beyond the rows the caller gave: no row is touched)
    if (lane == 0) { a.counters[(size_t)t * 5 + 3] = 1; a.stop[t] = 1u; }
    return;
  }
  const SmallSlice sl = small_slice(smem, P, S, U, wv);
  int2* const dom = sl.dom;
  uint32_t* const chg = sl.chg;
  uint32_t* const live = sl.live;
  uint32_t* const ent = sl.ent;
  uint32_t* const misc = sl.misc;
  auto wave_sync = [] { small_wave_sync(); };
  int32_t* const lb = a.lb + (size_t)t * a.capacity * V;
  int32_t* const ub = a.ub + (size_t)t * a.capacity * V;
  unsigned long long* const cnt = a.counters + (size_t)t * 5;
  unsigned long long nodes = cnt[0];
  const bool want_first = !BNB && a.first_solution != nullptr && cnt[1] == 0;  // the forest keeps each tree's FIRST solution
  uint32_t n_sol = 0, n_failed = 0, error = 0, wrote_first = 0;
  unsigned long long steps2 = 0, steps3 = 0;  // (per lane; reduced and flushed once)
  uint32_t acc_rounds = 0, acc_nodes = 0;
  Ctr ctr;
  const LdsDom dm{dom, 1u, chg, &misc[S_FAIL], 1u, &ctr, a.m.sums};

  if (lane < (uint32_t)S_WORDS) misc[lane] = 0;
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

  // ENUM: this tree's exclusion path and its rows' two words; n = the entries of the current node's list, path[0 .. n)
  pcp_excl* const path = ENUM ? a.path + (size_t)t * a.path_capacity : nullptr;
  uint32_t* const row_base = ENUM ? a.row_base + (size_t)t * a.capacity : nullptr;
  pcp_excl* const row_excl = ENUM ? a.row_excl + (size_t)t * a.capacity : nullptr;
  uint32_t n = 0;
  // a row whose list is in the path already: the left child nobody has popped, a node kept by error 1 — popping it again changes nothing
  auto store_row_words = [&](uint32_t r) {
    if (lane == 0) { row_base[r] = n; row_excl[r] = pcp_excl{kNoExcl, 0}; }
  };

  bool in_lds = false;  // the row on top of the stack is the LDS node (the left child of the node before) and has not been written
  for (uint32_t step = 0; step < a.n_steps && sp != 0 && !stop; ++step) {
    // ---- pop: row sp - 1 as (-lb, ub) cells ---------------------------------------------------------------------------------------------
    const uint32_t node = sp - 1;
    bool bad = false;
    if (lane == 0) misc[S_FAIL] = 0;
    if (ENUM && !in_lds) {
      // the row's list: the prefix it inherits, then its own entry.  (Wave-uniform loads: every lane reads the same two words)
      const uint32_t base = row_base[node];
      const pcp_excl own = row_excl[node];
      if (base > a.path_capacity || (own.var != kNoExcl && own.var >= V)) {
        // malformed: never used as an index.  Refused like a bound beyond +-(2^29 - 1): counted, popped, error 2, the sticky flag
        if (lane == 0) atomicMax(a.violation, 1u);
        ++nodes; error = 2; stop = 1; sp = node;
        break;
      }
      if (own.var != kNoExcl) {
        // 5: the exclusion path is full — nothing has been changed: the row stays on the stack, uncounted, and a caller that resumes
        // with a larger path runs it then (the contract of error 1)
        if (base == a.path_capacity) { error = 5; stop = 1; break; }
        if (lane == 0) path[base] = own;
        n = base + 1;
      } else {
        n = base;
      }
    }
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

    // ---- propagate: smallfix_kernel's rounds over the live units until a round narrows nothing or the node fails --------------------------
    bool failed = __ballot(bad) != 0;
    uint32_t rounds = 0, s2 = 0, s3 = 0;
    bool ex_open = false;  // ENUM: one of the node's exclusions is not entailed
    while (!failed) {
      ++rounds;
      const uint32_t before = ctr.narrow;
      if constexpr (ENUM) {
        ex_open = false;
        // the node's exclusions at the top of every round, lane-strided from global memory, exactly as smallexcl_kernel sweeps a CSR slice
        small_round(sh, P, Wu, sl, dm, lane, s2, s3, [&] {
          for (uint32_t i = lane; i < n; i += 64) {
            const pcp_excl e = path[i];
            if (e.var >= V) { dm.set_fail(); misc[S_OOB] = 1u; continue; }  // malformed: the tree is refused below
            const int K = e.value;
            const int2 c_ = dom[e.var];
            const int xl0 = -c_.x, xu0 = c_.y;
            int xl = xl0, xu = xu0;
            ++s2;
            // XNeqY(Identity(var), Constant(value))::propagate (x_neq_y.rs:82-93): a value is removed only at a bound
            if (xl0 == xu0) { if (xl0 == K) { dm.set_fail(); continue; } }
            else if (K == xl0) xl = xl0 + 1;
            else if (K == xu0) xu = xu0 - 1;
            if (xl > xl0) dm.raise_lb(e.var, xl);
            if (xu < xu0) dm.lower_ub(e.var, xu);
            ex_open |= !(K < xl || K > xu);  // is_subsumed() on what propagate() left (store.rs:166-175): True iff disjoint (x_neq_y.rs:71-73)
          }
        });
      } else {
        small_round(sh, P, Wu, sl, dm, lane, s2, s3, [] {});
      }
      wave_sync();
      failed = __builtin_amdgcn_readfirstlane(misc[S_FAIL]) != 0;
      if (!__ballot(ctr.narrow != before)) break;
    }
    steps2 += s2; steps3 += s3;
    acc_rounds += rounds ? rounds : 1;
    ++acc_nodes;
    if (ENUM && __builtin_amdgcn_readfirstlane(misc[S_OOB]) != 0) {  // a path entry with var >= n_vars: refused like the row's own (above)
      if (lane == 0) atomicMax(a.violation, 1u);
      ++nodes; error = 2; stop = 1; sp = node;
      break;
    }

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
    failed = failed || __ballot(emptied) != 0;
    // unlink_prop (store.rs:200-207): the last round narrowed nothing, so its `ent` is the entailment on the final domains
    if (!failed)
      for (uint32_t w = lane; w < Wu; w += 64) {
        const uint32_t left = live[w] & ~ent[w];
        live[w] = left;
        any_live |= left != 0;
      }
    // (ENUM: an exclusion that is not entailed keeps the node Unknown even when every unit is entailed)
    const bool unknown = !failed && __ballot(any_live || (ENUM && ex_open)) != 0;

    // ---- the step of dfs_step_kernel ----------------------------------------------------------------------------------------------------
    uint32_t new_sp = sp - 1;
    if (unknown) {
      for (int o = 32; o > 0; o >>= 1) key = min(key, (unsigned long long)__shfl_xor(key, o));
      if (key == ~0ull || sp >= a.capacity) {
        // 1: the stack is full — the node stays on the stack, propagated and uncounted: a caller that resumes with a larger stack runs it
        // again (idempotent) and counts it then.  3: Unknown, yet no variable with more than one value: the reference panics here
        // (first_smallest_var.rs:36)
        store_row(node);
        if (ENUM) store_row_words(node);
        error = key == ~0ull ? 3u : 1u; stop = 1;
        break;
      }
      const uint32_t var = (uint32_t)key;
      const int2 dv = dom[var];
      const int val = (int)(((long long)dv.y - (long long)dv.x) / 2);  // MiddleVal (middle_val.rs:25-27): `/` truncates toward zero like Rust's
      if constexpr (ENUM) {
        // Enumerate (enumerate.rs:47-60) on MiddleVal's or MinVal's value (min_val.rs:25-27: the lower bound).  A value the node has excluded
        // already is not chosen again (search.branch_enumerate, pcp_branch_device_excl): the nearest value of [lo, hi] without an entry on
        // `var`, m - d before m + d.  At a fixpoint neither bound of a variable is excluded — the sweep would have removed it — so a free
        // value always exists (there is no error code for "every value excluded") and MinVal's value is always free: under MinVal the
        // right child is always folded and the path never grows.  Every candidate inside [lo, hi] that is not free uses up an entry of its
        // own, so the search ends after at most n + 1 sweeps of n entries, whatever the width of the domain.
        const int lo = -dv.x, hi = dv.y;
        int v = a.val == PCP_VAL_MIN ? lo : val;
        if (a.val != PCP_VAL_MIN && n) {
          bool hit = false;
          for (uint32_t i = lane; i < n; i += 64) { const pcp_excl e = path[i]; hit |= e.var == var && e.value == v; }
          if (__ballot(hit)) {
            for (int d = 1;; ++d) {
              const int c0 = val - d, c1 = val + d;
              const bool in0 = c0 >= lo, in1 = c1 <= hi;
              if (!in0 && !in1) break;  // (not at a fixpoint, see above)
              bool h0 = false, h1 = false;
              for (uint32_t i = lane; i < n; i += 64) {
                const pcp_excl e = path[i];
                h0 |= e.var == var && e.value == c0;
                h1 |= e.var == var && e.value == c1;
              }
              if (in0 && !__ballot(h0)) { v = c0; break; }
              if (in1 && !__ballot(h1)) { v = c1; break; }
            }
          }
        }
        // Brancher (brancher.rs:52-71): the parent's row becomes the right child `x != v` — folded into the bound v sits at, else the
        // bounds as they are and the entry (var, v) for when the row is popped; either way it inherits the n entries of this node.  The
        // left child `x = v` goes on top, the path unchanged — it is the LDS node from here on
        const bool at_lb = v == lo, at_ub = v == hi;
        for (uint32_t u = lane; u < V; u += 64) {
          const int2 d = dom[u];
          lb[(size_t)node * V + u] = (u == var && at_lb) ? v + 1 : -d.x;
          ub[(size_t)node * V + u] = (u == var && at_ub && !at_lb) ? v - 1 : d.y;
          if (u == var) dom[u] = make_int2(-v, v);
        }
        if (lane == 0) { row_base[node] = n; row_excl[node] = (at_lb || at_ub) ? pcp_excl{kNoExcl, 0} : pcp_excl{var, v}; }
      } else {
        // Brancher (brancher.rs:52-71, binary_split.rs:46-57): the parent's row becomes the right child `x > val`; the left child `x <= val`
        // goes on top — it is the LDS node from here on
        for (uint32_t v = lane; v < V; v += 64) {
          const int2 d = dom[v];
          lb[(size_t)node * V + v] = (v == var) ? max(-d.x, val + 1) : -d.x;
          ub[(size_t)node * V + v] = d.y;
          if (v == var) dom[v].y = min(d.y, val);
        }
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
          if (ENUM) store_row_words(node);
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
    wave_sync();  // (the branch's LDS write, the live bits, and this tree's rows, before the next pop reads them)
  }

  if (in_lds) {  // the left child nobody has popped yet
    store_row(sp - 1);
    if (ENUM) store_row_words(sp - 1);
  }
  for (int o = 32; o > 0; o >>= 1) { steps2 += __shfl_down(steps2, o); steps3 += __shfl_down(steps3, o); ctr.narrow += __shfl_down(ctr.narrow, o); }
  if (lane == 0) {
    a.sp[t] = sp; a.stop[t] = stop;
    cnt[0] = nodes;
    if (n_sol) cnt[1] += n_sol;
    if (n_failed) cnt[2] += n_failed;
    if (error) cnt[3] = error;
    if (wrote_first) cnt[4] = 2;  // (dfs_step_kernel's flag: the first solution has been copied)
    pcp_stats* const stats = a.stats + (blockIdx.x & (kStatSlots - 1));
    const unsigned long long ev = steps2 + steps3;
    if (steps2) atomicAdd((unsigned long long*)&stats->steps, steps2);
    if (steps3) atomicAdd((unsigned long long*)&stats->steps3, steps3);
    if (ev) { atomicAdd((unsigned long long*)&stats->evaluated, ev); atomicAdd((unsigned long long*)&stats->full_evals, ev); }
    if (ctr.narrow) atomicAdd((unsigned long long*)&stats->narrowings, (unsigned long long)ctr.narrow);
    if (acc_rounds) atomicAdd((unsigned long long*)&stats->waves, (unsigned long long)acc_rounds);
    if (acc_nodes) atomicAdd((unsigned long long*)&stats->nodes, (unsigned long long)acc_nodes);
    if (n_failed) atomicAdd((unsigned long long*)&stats->failed_nodes, (unsigned long long)n_failed);
  }
}

template <bool BNB, bool ENUM, bool SINK>
hipError_t launch_smalldfs_as(const SmallDfsArgs& a, const LaunchPlan& p, hipStream_t stream) {
  hipError_t e;
  if (p.lds_bytes > 64 * 1024 &&
      (e = hipFuncSetAttribute(reinterpret_cast<const void*>(smalldfs_kernel<BNB, ENUM, SINK>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes)) != hipSuccess)
    return e;
  hipLaunchKernelGGL((smalldfs_kernel<BNB, ENUM, SINK>), dim3(p.grid), dim3(p.block), p.lds_bytes, stream, a);
  return hipGetLastError();
}

}  // namespace

size_t lds_bytes_smalldfs(uint32_t n_slots, uint32_t n_units, uint32_t n_recs, uint32_t waves) {
  const size_t b = small_shared_bytes(n_recs) + (size_t)waves * small_wave_bytes(n_slots, n_units);
  return b <= 160 * 1024 ? b : 0;
}

// p.block = 64 x the trees of a workgroup, p.grid = ceil(n_trees / those), p.lds_bytes = lds_bytes_smalldfs of them
hipError_t launch_smalldfs(const SmallDfsArgs& a, bool bnb, const LaunchPlan& p, hipStream_t stream) {
  if (!a.m.recs) return hipErrorInvalidValue;
  // the context's solution sink (pcp_solution_sink_set); the branch-and-bound entries refuse it
  const bool sink = a.sink.lb != nullptr;
  if (sink && (bnb || !a.sink.ub || !a.sink.count || !a.sink.capacity)) return hipErrorInvalidValue;
  if (a.row_base) {  // Enumerate: the rows' words are there (pcp_dfs_forest_device_small_enum)
    if (!a.row_excl || (a.path_capacity && !a.path)) return hipErrorInvalidValue;
    if (sink) return launch_smalldfs_as<false, true, true>(a, p, stream);
    return bnb ? launch_smalldfs_as<true, true, false>(a, p, stream) : launch_smalldfs_as<false, true, false>(a, p, stream);
  }
  if (sink) return launch_smalldfs_as<false, false, true>(a, p, stream);
  return bnb ? launch_smalldfs_as<true, false, false>(a, p, stream) : launch_smalldfs_as<false, false, false>(a, p, stream);
}

}  // namespace pcp
