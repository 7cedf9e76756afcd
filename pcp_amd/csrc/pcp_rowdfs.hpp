// pcp_rowdfs.hpp — the reference's search loop over Interval<i32> stores on the device, once, for both row-stack forests: what
// pcp_dfs_device does with three launches per node (a fixpoint kernel on the top row, then dfs_step_kernel), for MANY trees inside one
// launch.  formdfs_kernel (pcp_formdfs.hip: stores with formula units) and smalldfs_kernel (pcp_smalldfs.hip: small stores of plain
// propagators) both call row_dfs; each brings a NODE — its LDS slice and how a node is propagated and judged.  Device code only, all of it
// __forceinline__ templates: the two kernels are the loop specialised, not a call into it.  A tree is ONE WAVEFRONT in both (DESIGN.md
// §4.1, §4.6), so there is no team: a tree's steps are ordered by wave_sync(), and the trees of a workgroup never wait for each other.
//
// ≡ OneSolution / AllSolution<Propagation<Brancher<FirstSmallestVar, MiddleVal, BinarySplit>>> over a VectorStack (search/mod.rs:45-52,
// search/engine/one_solution.rs:92-105) under Monitor<Statistics, StopNode> (search/monitor.rs:19-68, search/stop_node.rs:47-62), and with
// BNB = true BranchAndBound around it (search/branch_and_bound.rs:64-84).
//
// Tree t works on slice t of a pcp_dfs_state laid out as for pcp_dfs_forest_device: a stack of (lb, ub) rows in HBM, rows [0, sp) open.  What
// a caller sees between two launches — sp, those rows, the counters, stop — is what pcp_dfs_device leaves after the same number of steps
// (dfs_step_kernel, pcp_kernels.hip, is the specification), so the host loop moves bottom rows between stacks and ranks as it does for the
// all-XNeqY forest.  Inside a launch:
//   - the left child is never read back: after the branch it IS the LDS node, with ub[var] lowered; its row is written only when the launch
//     ends with it on top of the stack;
//   - unit liveness is derived, never stored: an entailed unit stays entailed as domains shrink, so the descent to the left
//     child keeps the live bits; popping any other row sets every unit live, and the node's rounds unlink again what is entailed.
//
// ENUM = true: the same loop under Brancher<FirstSmallestVar, MiddleVal | MinVal, Enumerate> (search/branching/enumerate.rs:33-60).  The
// children are `x = v` and `x != v`; an interior `x != v` removes nothing from an Interval and stays with its node as a pcp_excl entry.  The
// batched search carries a CSR list per open node and copies it at every branch; a depth-first tree needs none of that: every open row of
// the stack is the right child of an ancestor of the current node, so its list is a PREFIX of the exclusions appended along the current
// path plus at most one entry of its own.  A tree keeps ONE path of entries in HBM and per stack row (row_base, row_excl) — how many path
// entries the row inherits and the entry appended when it is popped.  The current node's list is path[0 .. n), n wave-uniform in a
// register and re-derived from the top row at every launch; nothing is copied at a branch.  Entries are never filtered out of the path: an
// entry whose value lies outside [lb, ub] is entailed and stays so (domains only shrink below a node), and the value rule only looks
// inside [lb, ub] — the same tree as search.branch_enumerate's lists.  The exclusions are brancher state, not propagators of the store:
// the loop sweeps them at the top of every round (`sweep`) and a Node only has to run that callable.
//
// SINK = true (never with BNB): every solution is appended to the context's solution sink (SinkDev, pcp_neq.h) as a whole (lb, ub) row — a
// True node is a box, not a point.  A template flag, so that the instantiations without a sink are the code they were.
//
// A Node owns the pointers into its kernel's LDS slice — dom, chg, live, misc — the store's shape (V, S, U, const_val), `lane`, the
// per-lane counters and the LdsDom `dm` over them (its Ctr stands in the kernel beside the node: a struct that points into itself is
// not split into registers), names its words of misc (FAIL, WORDS and, if it can run under ENUM, OOB), and supplies
//   propagate(failed, sweep)   rounds until a round narrows nothing or the node fails, none if it `failed` on entry; sweep(steps2) at the
//                              top of every round; returns failed, adds to its round, node and step counters
//   any_live(failed)           does a unit remain subscribed (what keeps a node Unknown, store.rs:250-256)?  Per lane: the loop ballots
//   flush_stats(slot)          its counters into the pcp_stats slot, by every lane
// Integer bound work: no MFMA.
#pragma once
#include "pcp_device.hpp"
#include "pcp_neq.h"

namespace pcp {

namespace {

constexpr uint32_t kNoExcl = 0xFFFFFFFFu;  // row_excl[r].var: the row appends nothing when it is popped

// (the same two builtins as small_wave_sync, pcp_small.hpp, which the small store's round uses inside propagate())
__device__ __forceinline__ void wave_sync() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier(); }

// What a Node's flush_stats adds: its per-lane step counts (32 or 64 bits wide) and narrowings reduced over the wavefront, its rounds and nodes
template <class Steps>
__device__ __forceinline__ void flush_node_stats(pcp_stats* stats, uint32_t lane, Steps steps2, Steps steps3, uint32_t narrow, uint32_t rounds, uint32_t nodes) {
  for (int o = 32; o > 0; o >>= 1) { steps2 += __shfl_down(steps2, o); steps3 += __shfl_down(steps3, o); narrow += __shfl_down(narrow, o); }
  if (lane != 0) return;
  const unsigned long long ev = (unsigned long long)steps2 + steps3;
  if (steps2) atomicAdd((unsigned long long*)&stats->steps, (unsigned long long)steps2);
  if (steps3) atomicAdd((unsigned long long*)&stats->steps3, (unsigned long long)steps3);
  if (ev) { atomicAdd((unsigned long long*)&stats->evaluated, ev); atomicAdd((unsigned long long*)&stats->full_evals, ev); }
  if (narrow) atomicAdd((unsigned long long*)&stats->narrowings, (unsigned long long)narrow);
  if (rounds) atomicAdd((unsigned long long*)&stats->waves, (unsigned long long)rounds);
  if (nodes) atomicAdd((unsigned long long*)&stats->nodes, (unsigned long long)nodes);
}

template <bool BNB, bool ENUM, bool SINK, bool INPUT_ORDER, class Node>
__device__ __forceinline__ void row_dfs(const RowDfsArgs& d, const uint32_t t, Node& node) {
  static_assert(!(BNB && SINK), "branch and bound keeps tree_row; its entries refuse a sink");
  const uint32_t lane = node.lane;
  if (t >= d.n_trees) return;  // (wave-uniform: the other trees of the workgroup never wait for this one)
  uint32_t sp = d.sp[t], stop = d.stop[t];
  if (sp == 0 || stop) return;
  if (sp > d.capacity) {  // (a stack pointer beyond the rows the caller gave: no row is touched)
    if (lane == 0) { d.counters[(size_t)t * 5 + 3] = 1; d.stop[t] = 1u; }
    return;
  }
  const uint32_t V = node.V, S = node.S, Wv = (S + 31) >> 5, U = node.U, Wu = (U + 31) >> 5;
  int2* const dom = node.dom;
  uint32_t* const live = node.live;
  uint32_t* const misc = node.misc;
  const LdsDom& dm = node.dm;
  int32_t* const lb = d.lb + (size_t)t * d.capacity * V;
  int32_t* const ub = d.ub + (size_t)t * d.capacity * V;
  unsigned long long* const cnt = d.counters + (size_t)t * 5;
  unsigned long long nodes = cnt[0];
  const bool want_first = !BNB && d.first_solution != nullptr && cnt[1] == 0;  // the forest keeps each tree's FIRST solution
  uint32_t n_sol = 0, n_failed = 0, error = 0, wrote_first = 0;

  if (lane < (uint32_t)Node::WORDS) misc[lane] = 0;
  for (uint32_t w = lane; w < Wv; w += 64) node.chg[w] = 0;
  // The constants' cells (the Sum slots in between hold nothing: their domain is computed from the members).  Only a node that FAILS can
  // have narrowed one (Constant::update, term/constant.rs:49-52: a narrowed constant is an empty one), so they are written again after a
  // failed node only
  auto store_consts = [&] {
    for (uint32_t v = V + lane; v < S; v += 64) {
      const int c = (v - V >= dm.sums.count) ? node.const_val[v - V] : 0;
      dom[v] = make_int2(-c, c);
    }
  };
  store_consts();
  // the node in LDS: its lower bounds (a solution's row)
  auto store_lbs = [&](int32_t* out) { for (uint32_t v = lane; v < V; v += 64) out[v] = -dom[v].x; };
  // ... and the whole node, as row r of (lb, ub) rows
  auto store_row_to = [&](int32_t* out_lb, int32_t* out_ub, size_t r) {
    for (uint32_t v = lane; v < V; v += 64) { const int2 c = dom[v]; out_lb[r * V + v] = -c.x; out_ub[r * V + v] = c.y; }
  };

  // ENUM: this tree's exclusion path and its rows' two words; n = the entries of the current node's list, path[0 .. n)
  pcp_excl* const path = ENUM ? d.path + (size_t)t * d.path_capacity : nullptr;
  uint32_t* const row_base = ENUM ? d.row_base + (size_t)t * d.capacity : nullptr;
  pcp_excl* const row_excl = ENUM ? d.row_excl + (size_t)t * d.capacity : nullptr;
  uint32_t n = 0;
  // The node as row r of the stack.  ENUM: its list is in the path already — the left child nobody has popped, a node kept by error 1 or
  // 6 — so popping it again changes nothing
  auto store_row = [&](uint32_t r) {
    store_row_to(lb, ub, r);
    if constexpr (ENUM)
      if (lane == 0) { row_base[r] = n; row_excl[r] = pcp_excl{kNoExcl, 0}; }
  };
  // malformed input, never used as an index: the node is counted, popped and refused — error 2 and the sticky flag, as dfs_step_kernel does
  auto refuse = [&](uint32_t node_row) {
    if (lane == 0) atomicMax(d.violation, 1u);
    ++nodes; error = 2; stop = 1; sp = node_row;
  };

  bool in_lds = false;  // the row on top of the stack is the LDS node (the left child of the node before) and has not been written
  for (uint32_t step = 0; step < d.n_steps && sp != 0 && !stop; ++step) {
    // ---- pop: row sp - 1 as (-lb, ub) cells ---------------------------------------------------------------------------------------------
    const uint32_t top = sp - 1;
    bool bad = false;
    if (lane == 0) misc[Node::FAIL] = 0;
    if (ENUM && !in_lds) {
      // the row's list: the prefix it inherits, then its own entry.  (Wave-uniform loads: every lane reads the same two words)
      const uint32_t base = row_base[top];
      const pcp_excl own = row_excl[top];
      if (base > d.path_capacity || (own.var != kNoExcl && own.var >= V)) { refuse(top); break; }
      if (own.var != kNoExcl) {
        // 5: the exclusion path is full — nothing has been changed: the row stays on the stack, uncounted, and a caller that resumes
        // with a larger path runs it then (the contract of error 1)
        if (base == d.path_capacity) { error = 5; stop = 1; break; }
        if (lane == 0) path[base] = own;
        n = base + 1;
      } else {
        n = base;
      }
    }
    if (!in_lds) {
      bool wide = false;
      for (uint32_t v = lane; v < V; v += 64) {
        const int l = lb[(size_t)top * V + v], u = ub[(size_t)top * V + v];
        bad |= l > u;
        wide |= (l < -kBoundMax) | (l > kBoundMax) | (u < -kBoundMax) | (u > kBoundMax);
        dom[v] = make_int2(-l, u);
      }
      for (uint32_t w = lane; w < Wu; w += 64) live[w] = (w == Wu - 1 && (U & 31u)) ? (1u << (U & 31u)) - 1u : 0xFFFFFFFFu;
      // a bound beyond +-(2^29 - 1): refused, not wrapped (pcp_hip.h)
      if (__ballot(wide)) { refuse(top); break; }
    }
    in_lds = false;
    wave_sync();
    if (BNB) {
      // the bound propagator of BranchAndBound, folded (branch_and_bound.rs:64-84): var < best resp. var > best on the incumbent as it is
      // NOW.  "No solution yet" (+-(PCP_BOUND_MAX + 1)) narrows nothing.  The fold stays in the node: the right child inherits it and
      // folds again when it is popped (search._IntervalRows.propagate)
      const long long best = __hip_atomic_load(d.obj_best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      int2 c = dom[d.obj_var];
      const long long lim = (long long)kBoundMax + 1;
      if (d.obj_mode == PCP_MINIMIZE) c.y = (int)min((long long)c.y, max(best - 1, -lim));
      else c.x = (int)min((long long)c.x, -min(best + 1, lim));
      bad |= -c.x > c.y;  // a node the fold empties is a node and a failed node, and no unit runs
      if (lane == 0) dom[d.obj_var] = c;
      wave_sync();
    }

    // ---- propagate: the node's rounds over its live units; ENUM: the node's exclusions at the top of every round, lane-strided from global
    //      memory, exactly as smallexcl_kernel sweeps a CSR slice ---------------------------------------------------------------------------
    bool ex_open = false;  // ENUM: one of the node's exclusions is not entailed
    bool failed = __ballot(bad) != 0;
    if constexpr (ENUM) {
      failed = node.propagate(failed, [&](uint32_t& steps2) {
        ex_open = false;
        for (uint32_t i = lane; i < n; i += 64) {
          const pcp_excl e = path[i];
          if (e.var >= V) { dm.set_fail(); misc[Node::OOB] = 1u; continue; }  // malformed: the tree is refused below
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
      });
      // a path entry with var >= n_vars: refused like the row's own (above)
      if (__builtin_amdgcn_readfirstlane(misc[Node::OOB]) != 0) { refuse(top); break; }
    } else {
      failed = node.propagate(failed, [](uint32_t&) {});
    }

    // ---- Consistency::consistency (store.rs:250-256): False if a propagate failed, True if no subscription remains, else Unknown; and the
    //      key of FirstSmallestVar (first_smallest_var.rs:30-39): the smallest size > 1, the lowest index on a tie — or, under InputOrder
    //      (input_order.rs:30-39; INPUT_ORDER), the lowest index of size > 1: the key without the size -----------------------------------------
    bool emptied = false;
    unsigned long long key = ~0ull;
    for (uint32_t v = lane; v < V; v += 64) {
      const int2 c = dom[v];
      emptied |= -c.x > c.y;
      const unsigned long long size = (unsigned long long)((long long)c.y + (long long)c.x + 1);
      if (size > 1) key = min(key, INPUT_ORDER ? (unsigned long long)v : (size << 32) | v);
    }
    failed = failed || __ballot(emptied) != 0;
    // (ENUM: an exclusion that is not entailed keeps the node Unknown even when every unit is entailed)
    const bool any_live = node.any_live(failed);
    const bool unknown = !failed && __ballot(any_live || (ENUM && ex_open)) != 0;

    // ---- the step of dfs_step_kernel ----------------------------------------------------------------------------------------------------
    uint32_t new_sp = sp - 1;
    if (unknown) {
      for (int o = 32; o > 0; o >>= 1) key = min(key, (unsigned long long)__shfl_xor(key, o));
      if (key == ~0ull || sp >= d.capacity) {
        // 1: the stack is full — the node stays on the stack, propagated and uncounted: a caller that resumes with a larger stack runs it
        // again (idempotent) and counts it then.  3: Unknown, yet no variable with more than one value: the reference panics here
        // (first_smallest_var.rs:36)
        store_row(top);
        error = key == ~0ull ? 3u : 1u; stop = 1;
        break;
      }
      const uint32_t var = (uint32_t)key;
      const int2 dv = dom[var];
      const int val = (int)(((long long)dv.y - (long long)dv.x) / 2);  // MiddleVal (middle_val.rs:25-27): `/` truncates toward zero like Rust's
      if constexpr (ENUM) {
        // Enumerate (enumerate.rs:47-60) on MiddleVal's or MinVal's value (min_val.rs:25-27: the lower bound).  A value the node has excluded
        // already is not chosen again (search.branch_enumerate, pcp_branch_device_excl): the nearest value of [lo, hi] without an entry on
        // `var`, m - k before m + k.  At a fixpoint neither bound of a variable is excluded — the sweep would have removed it — so a free
        // value always exists (there is no error code for "every value excluded") and MinVal's value is always free: under MinVal the
        // right child is always folded and the path never grows.  Every candidate inside [lo, hi] that is not free uses up an entry of its
        // own, so the search ends after at most n + 1 sweeps of n entries, whatever the width of the domain.
        const int lo = -dv.x, hi = dv.y;
        int v = d.val == PCP_VAL_MIN ? lo : val;
        if (d.val != PCP_VAL_MIN && n) {
          bool hit = false;
          for (uint32_t i = lane; i < n; i += 64) { const pcp_excl e = path[i]; hit |= e.var == var && e.value == v; }
          if (__ballot(hit)) {
            for (int k = 1;; ++k) {
              const int c0 = val - k, c1 = val + k;
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
          const int2 c = dom[u];
          lb[(size_t)top * V + u] = (u == var && at_lb) ? v + 1 : -c.x;
          ub[(size_t)top * V + u] = (u == var && at_ub && !at_lb) ? v - 1 : c.y;
          if (u == var) dom[u] = make_int2(-v, v);
        }
        if (lane == 0) { row_base[top] = n; row_excl[top] = (at_lb || at_ub) ? pcp_excl{kNoExcl, 0} : pcp_excl{var, v}; }
      } else {
        // Brancher (brancher.rs:52-71, binary_split.rs:46-57): the parent's row becomes the right child `x > val`; the left child `x <= val`
        // goes on top — it is the LDS node from here on
        for (uint32_t v = lane; v < V; v += 64) {
          const int2 c = dom[v];
          lb[(size_t)top * V + v] = (v == var) ? max(-c.x, val + 1) : -c.x;
          ub[(size_t)top * V + v] = c.y;
          if (v == var) dom[v].y = min(c.y, val);
        }
      }
      new_sp = sp + 1;
      in_lds = true;
    }
    if constexpr (SINK) {
      // A solution draws its ticket BEFORE it is counted (the limit node, `nodes + 1` at the limit, is no solution and draws none).  6: the
      // sink is full — the node stays on the stack, propagated and uncounted, and a caller that drains the sink and resumes runs it again
      // (idempotent), counts it then and appends it then (the contract of error 1)
      if (!failed && !unknown && !(d.node_limit && nodes + 1 >= d.node_limit)) {
        uint32_t slot = 0;
        if (lane == 0) slot = __hip_atomic_fetch_add(d.sink.count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        slot = __builtin_amdgcn_readfirstlane(slot);
        if (slot >= d.sink.capacity) {
          store_row(top);
          error = kDfsSinkFull; stop = 1;
          break;
        }
        store_row_to(d.sink.lb, d.sink.ub, slot);
        if (lane == 0 && d.sink.tree) d.sink.tree[slot] = t;
      }
    }
    // Monitor<Statistics, StopNode>: the node that reaches the limit is a node, but neither a solution nor a failure (stop_node.rs:57-62, 90-97)
    ++nodes;
    const bool last = d.node_limit && nodes >= d.node_limit;
    if (!failed && !unknown && !last) {
      ++n_sol;
      if (BNB) {
        // the incumbent becomes var.lower() in both modes; within a tree every solution beats the one before
        const int value = -dom[d.obj_var].x;
        if (d.tree_row) store_lbs(d.tree_row + (size_t)t * V);
        if (lane == 0) {
          d.tree_best[t] = value;
          if (d.obj_mode == PCP_MINIMIZE) atomicMin(d.obj_best, value); else atomicMax(d.obj_best, value);
        }
      } else {
        if (want_first && !wrote_first) { store_lbs(d.first_solution + (size_t)t * V); wrote_first = 1; }
        if (d.stop_on_solution) stop = 1;
      }
    } else if (failed && !last) {
      ++n_failed;
    }
    if (failed) store_consts();
    if (last) stop = 1;
    sp = new_sp;
    wave_sync();  // (the branch's LDS write, the live bits, and this tree's rows, before the next pop reads them)
  }

  if (in_lds) store_row(sp - 1);  // the left child nobody has popped yet
  pcp_stats* const stats = d.stats + (blockIdx.x & (kStatSlots - 1));
  node.flush_stats(stats);
  if (lane == 0) {
    d.sp[t] = sp; d.stop[t] = stop;
    cnt[0] = nodes;
    if (n_sol) cnt[1] += n_sol;
    if (n_failed) cnt[2] += n_failed;
    if (error) cnt[3] = error;
    if (wrote_first) cnt[4] = 2;  // (dfs_step_kernel's flag: the first solution has been copied)
    if (n_failed) atomicAdd((unsigned long long*)&stats->failed_nodes, (unsigned long long)n_failed);
  }
}

}  // namespace

}  // namespace pcp
