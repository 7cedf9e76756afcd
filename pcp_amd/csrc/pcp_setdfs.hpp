// pcp_setdfs.hpp — the reference's search loop over FDSpace on the device, once, for both set-mode forests:
// OneSolution / AllSolution<Propagation<Brancher<FirstSmallestVar, MiddleVal | MinVal, BinarySplit | Enumerate>>> (search/mod.rs:45-52) over
// VStoreSet = VStoreTrail<IntervalSet<i32>> (variable/mod.rs:38), optionally inside BranchAndBound<..> (branch_and_bound.rs:64-84).
// setdfs_kernel (pcp_set.hip: stores of records) and setformdfs_kernel (pcp_setformdfs.hip: stores with formula units) both call
// trail_dfs; each brings a TEAM — who runs a tree — and a NODE — how a node is loaded, propagated and judged.  Device code only, all of
// it __forceinline__ templates: the two kernels are the loop specialised, not a call into it.
//
// The reference restores a node by undoing a TRAIL (variable/memory/trail_memory.rs:100-104); so does this loop: the current node never
// leaves LDS, every narrowing appends (word index, variable, removed bits lo, hi) to the tree's trail in HBM (SetDomT<true>::log), a
// backtrack ORs the bits back down to the level's mark and applies the right branch.  A child differs from its parent's fixpoint in the
// branched variable only, so only that variable is marked changed; `pending` names it (kDfsFull: a root, not propagated at all).
// Exactly the reference's left-first order within a tree; several trees = the subtrees of an open-node frontier.
//   tree[4]  = levels, trail length, pending, finished | given << 8 (given: its oldest levels whose right branch went to another tree)
//   a level  = (variable, value, trail mark, kLevelGiven | kLevelEnum)
// setdfs_split_kernel (pcp_set.hip) hands work between the trees of either forest on this state alone.
//
// ENUM: the loop under Enumerate (enumerate.rs:47-60) — a level is `x = v, then x != v`, v the member of the set nearest to the selector's
// value (a.val_mode) — instead of BinarySplit on MiddleVal.  A template parameter, not a scalar branch.
//
// BNB: the forest shares ONE incumbent, a device int32 (a.obj_best).  On entering a node — before its propagation — the bound  var < best
// (minimize) /  var > best  (maximize) is folded into the objective variable's set through restrict_var: XLessY(var, Constant(best)) narrows
// once and is then entailed (pcp_bnb.hip), the removal is trailed and marks the variable changed, and a fold that empties the set fails the
// node on its first bounds scan like any other empty set (a node and a failure, as the reference counts it).  Before any solution the
// incumbent is the "no solution yet" value of pcp_hip.h, which lies outside every set: the fold is a no-op.  The fold stands where a
// synchronisation already follows the branch restriction (descend, backtrack) and once at launch start, for the node the tree enters first:
// a root, a node persisted by the launch before, or one handed over by setdfs_split_kernel.  Its trail entries come after the level's mark,
// so a backtrack undoes them and the right child folds again against the incumbent of that moment; the incumbent only improves, so nothing
// a fold removed could have stayed.  The trail bound of the plain loop holds: a fold entry, like every other, takes at least one value out
// of a set and is popped before that value can return.  On a solution v = lower(var) beats every earlier value of this tree (the node
// passed the fold): the tree keeps v and the node's lower bounds (a.tree_best, a.tree_row) and then lowers / raises the incumbent atomically
// — another tree may hold a better one already, so the winner's row is chosen on the host among the trees whose value equals the final
// incumbent.  There is no stop-on-solution and no first solution: branch and bound runs to the end (or to the node limit).
//
// SINK = true (never with BNB): every solution is appended to the context's set solution sink (SetSinkDev, pcp_internal.h) as the WHOLE
// node, V x set_words words — a True node over sets is a product of sets, not a point.  A template flag, so that the instantiations without
// a sink are the code they were.  A solution (never the limit node, which is none) draws a ticket BEFORE it is counted: the leader's
// atomicAdd on *count at agent scope, made uniform by team.broadcast_ticket before any lane uses it as an address.  slot < capacity: the
// node goes from LDS to row `slot` (copy_node: plain vector stores, 16 bytes at a time where the row allows it), tree[slot] = t, and the
// step goes on as without a sink.  slot >= capacity: error 6, "sink full", the contract of error 1 — nothing is counted, the reserved node
// goes back to the forest's counter, pending = kDfsFull, and the final persist writes the node, AT ITS FIXPOINT, with the trail and the
// levels untouched.  A relaunch loads it and propagates everything, which at a fixpoint narrows nothing and appends nothing to the trail
// (in setformdfs_kernel every unit is live at launch start anyway), finds the same status, draws a ticket that fits and counts and appends
// the node once.  Why no counter of any tree differs from a run whose sink never fills: the handed-back node was not counted (c_nodes,
// c_sols untouched, its reservation returned), its second run leaves the sets, the trail and the levels as the first did, so the tree goes
// on from exactly the state it would have had; other trees see the raised stop word only between nodes, as on any launch end, and their
// nodes do not depend on when they run.  A tree stopped by error 6 is an ordinary donor for setdfs_split_kernel: its levels and trail
// describe its current node, as after any launch.
//
// A Team gives: rank, size, lane; leader() (one thread); wave_wide() (the one wavefront that does the single-variable, wave-wide steps:
// restriction, fold, value); sync(); broadcast() of one or two words from the leader, broadcast_ticket() of the sink's slot; min_of_waves().  Values every thread of a team reads
// from the same address (tree[], a level) are held once per wavefront (uniform()).
// A Node owns the pointers into its kernel's LDS carve — bits, bnd, misc, touched (mask_words words), mark_mask(): the mask a restriction
// marks — and the per-thread `narrow`, and supplies
//   load(gbits)            the tree's node into LDS, masks and misc zeroed, synchronised
//   begin(pending)         launch start, after S_TRAILLEN is set and before the fold;  begun(): after the fold and its sync
//   propagate(pending)     to the fixpoint or the failure; returns whether the rounds ran away
//   status()               {failed, open} (store.rs:250-256), synchronised;  branch_key(): the variable selector's key for an open node
//   backtracking()         before the trail and the levels are read back;
//   backtracked()          after the bounds of the touched variables, before the synchronisation that precedes the right branch
//   end_node()             before the synchronisation that ends a node
//   flush_stats(slot, nodes)
// Synchronisation: every LDS word one thread writes and another reads has a team.sync() between the two.  The loop itself holds: one after
// a reservation (inside broadcast, every kDfsChunk nodes), one inside the first-solution broadcast, two in a backtrack (undo | bounds and
// S_TRAILLEN | right branch) and one at a node's end (the restriction's bits, marks and trail length | the next node's rounds); everything
// else is the Node's.  For a workgroup each is a barrier, so the loop adds none per node to what propagate() and status() need.
#pragma once
#include "pcp_setdom.hpp"

namespace pcp {

namespace {

__device__ __forceinline__ uint32_t uniform(uint32_t x) { return __builtin_amdgcn_readfirstlane(x); }

// One tree per workgroup: __syncthreads, broadcasts through the S_CTL words of `misc`, a minimum across wavefronts through `wave_min`
// (one 8-byte word per wavefront that is idle whenever min_of_waves runs).
struct WorkgroupTeam {
  uint32_t rank, size, lane, wave, n_waves;
  uint32_t* ctl;
  unsigned long long* wave_min;
  __device__ __forceinline__ WorkgroupTeam(uint32_t* misc, unsigned long long* wave_min_)
      : rank(threadIdx.x), size(blockDim.x), lane(threadIdx.x & 63), wave(uniform(threadIdx.x >> 6)), n_waves(blockDim.x >> 6), ctl(misc + S_CTL), wave_min(wave_min_) {}
  __device__ __forceinline__ bool leader() const { return rank == 0; }
  __device__ __forceinline__ bool wave_wide() const { return wave == 0; }
  __device__ __forceinline__ void sync() const { __syncthreads(); }
  __device__ __forceinline__ uint32_t broadcast(uint32_t x) const {
    if (leader()) ctl[1] = x;
    sync();
    return ctl[1];
  }
  __device__ __forceinline__ void broadcast(uint32_t& x, uint32_t& y) const {
    if (leader()) { ctl[0] = x; ctl[2] = y; }
    sync();
    x = ctl[0]; y = ctl[2];
  }
  // (a word of its own: the first-solution broadcast may follow with no barrier between, and must not overwrite a slot still being read)
  __device__ __forceinline__ uint32_t broadcast_ticket(uint32_t x) const {
    if (leader()) ctl[3] = x;
    sync();
    return uniform(ctl[3]);
  }
  __device__ __forceinline__ unsigned long long min_of_waves(unsigned long long key) const {  // key: each wavefront's own minimum
    if (lane == 0) wave_min[wave] = key;
    sync();
    key = wave_min[0];
    for (uint32_t w = 1; w < n_waves; ++w) key = min(key, wave_min[w]);
    return key;
  }
};

// One tree per wavefront, the trees of a workgroup independent of each other: there is no workgroup barrier, a tree's steps are ordered
// by a workgroup-scope fence and a wave barrier, broadcasts are shuffles.
struct WavefrontTeam {
  uint32_t rank, size, lane;
  __device__ __forceinline__ WavefrontTeam() : rank(threadIdx.x & 63), size(64), lane(threadIdx.x & 63) {}
  __device__ __forceinline__ bool leader() const { return lane == 0; }
  __device__ __forceinline__ bool wave_wide() const { return true; }
  __device__ __forceinline__ void sync() const { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier(); }
  __device__ __forceinline__ uint32_t broadcast(uint32_t x) const { return __shfl(x, 0); }
  __device__ __forceinline__ void broadcast(uint32_t& x, uint32_t& y) const { x = __shfl(x, 0); y = __shfl(y, 0); }
  __device__ __forceinline__ uint32_t broadcast_ticket(uint32_t x) const { return uniform(x); }  // (lane 0 is the leader and is active)
  __device__ __forceinline__ unsigned long long min_of_waves(unsigned long long key) const { return key; }
};

// n 8-byte words between a tree's row in HBM and its node in LDS, 16 bytes at a time where the row allows it
template <class Team>
__device__ __forceinline__ void copy_node(const Team& team, unsigned long long* dst, const unsigned long long* src, uint32_t n) {
  if (!(n & 1u) && !(((size_t)dst | (size_t)src) & 15)) {
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    uint4* d4 = reinterpret_cast<uint4*>(dst);
    for (uint32_t i = team.rank; i < n / 2; i += team.size) d4[i] = s4[i];
  } else {
    for (uint32_t i = team.rank; i < n; i += team.size) dst[i] = src[i];
  }
}

// FirstSmallestVar on sets: the variable of minimal CARDINALITY > 1, first index (first_smallest_var.rs:30-39 on Domain::size()) — a
// popcount per variable, a minimum over the key size << 32 | v.  ~0: every variable is assigned.  Under InputOrder (var_select, wave-uniform;
// input_order.rs:30-39) the first variable of cardinality > 1: the same minimum with the size masked out of the key.
template <class Team>
__device__ __forceinline__ unsigned long long first_smallest_var(const Team& team, const unsigned long long* bits, uint32_t V, uint32_t sw, uint32_t var_select) {
  const uint32_t size_mask = var_size_mask(var_select);
  unsigned long long key = ~0ull;
  for (uint32_t v = team.rank; v < V; v += team.size) {
    unsigned long long size = 0;
    for (uint32_t k = 0; k < sw; ++k) size += (unsigned long long)__popcll(bits[(size_t)v * sw + k]);
    if (size > 1) key = min(key, var_key(size, v, size_mask));
  }
  for (int o = 32; o > 0; o >>= 1) key = min(key, (unsigned long long)__shfl_xor(key, o));
  return team.min_of_waves(key);
}

struct NodeStatus { bool failed, open; };

template <bool ENUM, bool BNB, bool SINK, class Team, class Node>
__device__ __forceinline__ void trail_dfs(const SetDfsArgs& a, const SetSinkDev& sink, const uint32_t t, const Team team, Node& node) {
  static_assert(!(BNB && SINK), "branch and bound keeps tree_row; its entries refuse a set sink");
  uint32_t* const tree = a.tree + (size_t)t * 4;
  if (uniform(tree[3]) & 1u) return;  // this tree is finished
  uint32_t n_levels = uniform(tree[0]), pending = uniform(tree[2]);
  const uint32_t given0 = uniform(tree[3]) >> 8;  // its oldest levels whose right branch went to another tree (setdfs_split_kernel)
  const uint32_t V = a.m.n_vars, sw = a.set_words, lane = team.lane;
  uint4* const trail = a.trail + (size_t)t * a.trail_cap;
  uint4* const levels = a.levels + (size_t)t * a.level_cap;
  unsigned long long* const gbits = reinterpret_cast<unsigned long long*>(a.bits) + (size_t)t * V * sw;
  unsigned long long* const bits = node.bits;
  int2* const bnd = node.bnd;
  uint32_t* const misc = node.misc;
  uint32_t* const touched = node.touched;

  // a branch constraint folded into the variable's set: the values lo..hi leave it — one lane per word of the wave-wide wavefront (one
  // thread doing the up to set_words atomics and trail entries in turn was a quarter of a cheap node), every removal trailed
  auto restrict_var = [&](uint32_t var, long long lo, long long hi) {
    if (!team.wave_wide()) return;
    const SetDomT<true> dm{bits, bnd, a.m.const_val, V, sw, a.base, node.mark_mask(), misc, &node.narrow, trail, &misc[S_TRAILLEN], a.trail_cap};
    long long b0 = lo - a.base, b1 = hi - a.base;
    if (b0 < 0) b0 = 0;
    if (b1 >= (long long)sw * 64) b1 = (long long)sw * 64 - 1;
    bool changed = false;
    for (long long k = (b0 >> 6) + lane; b0 <= b1 && k <= (b1 >> 6); k += 64) {
      unsigned long long m = ~0ull;
      if (k == (b0 >> 6)) m &= ~0ull << (b0 & 63);
      if (k == (b1 >> 6)) m &= ~0ull >> (63 - (b1 & 63));
      const unsigned long long gone = atomicAnd(&bits[(size_t)var * sw + k], ~m) & m;
      if (gone) { changed = true; dm.log(var, var * sw + (uint32_t)k, gone); }
    }
    if (__ballot(changed) != 0 && lane == 0) dm.mark(var);
  };
  // BNB: the bound folded into the objective's set — the values >= best (minimize) / <= best (maximize) leave it
  auto fold_bound = [&]() {
    if (!team.wave_wide()) return;
    const long long best = (long long)__hip_atomic_load(a.obj_best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (a.obj_mode == PCP_MINIMIZE) restrict_var(a.obj_var, best, 1ll << 40);
    else restrict_var(a.obj_var, -(1ll << 40), best);
  };

  // ---- the tree's current node into LDS; under BNB the node this launch enters first against the incumbent of now ----------------------
  node.load(gbits);
  if (team.leader()) misc[S_TRAILLEN] = tree[1];
  node.begin(pending);
  if constexpr (BNB) { fold_bound(); team.sync(); }
  node.begun();

  unsigned long long c_nodes = 0, c_sols = 0, c_fail = 0;
  uint32_t c_err = 0;
  bool finished = false;
  uint32_t reserved = 0;       // nodes this tree may still run before it asks the forest's counter again
  bool res_has_last = false;   // ... the last of which is the node that reaches the limit

  for (uint32_t step = 0; step < a.n_steps; ++step) {
    // ---- may this node run?  The stop flag of the forest and the node limit of all trees together (StopNode, stop_node.rs:57-62): nodes
    // are reserved kDfsChunk at a time from the forest's counter (two device-scope atomics and a barrier per node were a fifth of a cheap
    // node); what a tree does not use goes back when the launch ends.  The node that reaches the limit is explored and counted, but
    // StopNode replaces its status by EndOfSearch (stop_node.rs:55-62): it is neither a solution nor a failure.
    if (reserved == 0) {
      uint32_t got = 0, has_last = 0;
      if (team.leader() && !__hip_atomic_load(a.stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
        const unsigned long long want = min((unsigned long long)kDfsChunk, (unsigned long long)(a.n_steps - step));
        const unsigned long long old = atomicAdd(a.total_nodes, want);
        if (!a.node_limit) got = (uint32_t)want;
        else if (old >= a.node_limit) atomicAdd(a.total_nodes, 0ull - want);
        else {
          got = (uint32_t)min(want, a.node_limit - old);
          if (got < want) atomicAdd(a.total_nodes, 0ull - (want - got));
          has_last = old + got >= a.node_limit ? 1u : 0u;
        }
      }
      team.broadcast(got, has_last);
      reserved = got;
      res_has_last = has_last != 0;
      if (!reserved) break;
    }
    --reserved;
    const bool last = res_has_last && reserved == 0;

    const bool runaway = node.propagate(pending);
    const NodeStatus st = node.status();
    const uint32_t tlen = uniform(misc[S_TRAILLEN]);
    if (uniform(misc[S_TRAILOVF])) { c_err = 4; break; }  // the trail is full: the tree cannot be restored any more (terminal)
    if (runaway) { c_err = 5; break; }
    ++c_nodes;
    bool descend = false;
    if (st.failed) {
      if (!last) ++c_fail;
    } else if (!st.open && last) {
    } else if (!st.open) {  // a solution (monitor.rs:19-68)
      if constexpr (SINK) {
        // the ticket comes first: a node that finds the sink full is handed back uncounted, at its fixpoint (the contract of error 1)
        uint32_t slot = 0;
        if (team.leader()) slot = __hip_atomic_fetch_add(sink.count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        slot = team.broadcast_ticket(slot);
        if (slot >= sink.capacity) { c_err = kSetDfsSinkFull; --c_nodes; pending = kDfsFull; if (team.leader()) atomicAdd(a.total_nodes, ~0ull); break; }
        copy_node(team, reinterpret_cast<unsigned long long*>(sink.bits) + (size_t)slot * V * sw, bits, V * sw);
        if (team.leader() && sink.tree) sink.tree[slot] = t;
        // (the backtrack below writes `bits`; with first_solution the barrier of its broadcast stands between the copy and those writes)
        if (!a.first_solution) team.sync();
      }
      ++c_sols;
      if constexpr (BNB) {
        // the incumbent is var.lower() in both modes (branch_and_bound.rs:73-77): the tree keeps the value and the row, then lowers / raises
        // the forest's incumbent (another tree may hold a better one already)
        const int v = bnd[a.obj_var].x;
        if (a.tree_row)
          for (uint32_t u = team.rank; u < V; u += team.size) a.tree_row[(size_t)t * V + u] = bnd[u].x;
        if (team.leader()) {
          a.tree_best[t] = v;
          // (the old value is used, so the atomic has been performed before the backtrack below reads the incumbent for its fold)
          const int old = a.obj_mode == PCP_MINIMIZE ? __hip_atomic_fetch_min(a.obj_best, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                                     : __hip_atomic_fetch_max(a.obj_best, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          misc[S_CTL + 1] = (uint32_t)old;
        }
      } else if (a.first_solution) {  // the first one of the forest is kept
        uint32_t won = 0;
        if (team.leader()) won = atomicCAS(a.solution_flag, 0u, 1u) == 0u ? 1u : 0u;
        if (team.broadcast(won))
          for (uint32_t v = team.rank; v < V; v += team.size) a.first_solution[v] = bnd[v].x;
      }
      if (a.stop_on_solution && team.leader()) atomicExch(a.stop, 1u);
    } else {
      // Brancher<FirstSmallestVar | InputOrder, MiddleVal | MinVal, BinarySplit | Enumerate>::enter on sets
      const unsigned long long key = node.branch_key();
      if (key == ~0ull) { c_err = 3; --c_nodes; if (team.leader()) atomicAdd(a.total_nodes, ~0ull); break; }  // Unknown, yet nothing to branch on: the reference panics
      if (n_levels >= a.level_cap) { c_err = 1; --c_nodes; pending = kDfsFull; if (team.leader()) atomicAdd(a.total_nodes, ~0ull); break; }
      const uint32_t var = (uint32_t)key;
      if (team.wave_wide()) {
        const int2 d = bnd[var];
        if constexpr (ENUM) {
          // MinVal: lower() (min_val.rs:25-27), a member; MiddleVal: (lower + upper) / 2 (middle_val.rs:25-27) or, when that is a hole of
          // the set, the member nearest to it, the lower one first: one lane per word, a minimum across the lanes
          long long v = d.x;
          if (a.val_mode != PCP_VAL_MIN) {
            const long long m = ((long long)d.x + (long long)d.y) / 2;
            unsigned long long nk = ~0ull;
            for (uint32_t k = lane; k < sw; k += 64) nk = min(nk, nearest_member_key(bits[(size_t)var * sw + k], (long long)a.base + 64ll * (long long)k, m));
            for (int o = 32; o > 0; o >>= 1) nk = min(nk, (unsigned long long)__shfl_xor(nk, o));
            v = nearest_member_value(nk, m);
          }
          if (team.leader()) levels[n_levels] = make_uint4(var, (uint32_t)(int)v, tlen, kLevelEnum);
          // the left child x = v (enumerate.rs:47-53): everything below v and everything above it leaves the set
          restrict_var(var, d.x, v - 1);
          restrict_var(var, v + 1, d.y);
        } else {
          const int val = (int)(((long long)d.x + (long long)d.y) / 2);  // MiddleVal (middle_val.rs:25-27)
          if (team.leader()) levels[n_levels] = make_uint4(var, (uint32_t)val, tlen, 0u);
          restrict_var(var, (long long)val + 1, d.y);  // the left child x <= val (binary_split.rs:46-57)
        }
        if constexpr (BNB) fold_bound();
      }
      ++n_levels;
      pending = var;
      descend = true;
    }
    if (!descend) {
      // ---- backtrack: the deepest level whose right branch is still open (a level whose right branch was given to another tree is undone
      // like any other and skipped) ----------------------------------------------------------------------------------------------------------
      node.backtracking();
      uint4 lv = make_uint4(0u, 0u, 0u, kLevelGiven);
      uint32_t from = tlen;
      while (n_levels) {
        --n_levels;
        const uint4 q = levels[n_levels];
        lv = make_uint4(uniform(q.x), uniform(q.y), uniform(q.z), uniform(q.w));
        for (uint32_t i = lv.z + team.rank; i < from; i += team.size) {
          const uint4 e = trail[i];
          atomicOr(&bits[e.x], ((unsigned long long)e.w << 32) | e.z);
          atomicOr(&touched[e.y >> 5], 1u << (e.y & 31u));
        }
        from = lv.z;
        if (!(lv.w & kLevelGiven)) break;
      }
      if (lv.w & kLevelGiven) { finished = true; break; }  // nothing left that is this tree's
      team.sync();
      if (team.leader()) { misc[S_TRAILLEN] = from; misc[S_FAIL] = 0; }
      for (uint32_t v = team.rank; v < V; v += team.size)
        if ((touched[v >> 5] >> (v & 31u)) & 1u) bnd[v] = scan_bounds(bits + (size_t)v * sw, sw, a.base);
      node.backtracked();
      team.sync();
      for (uint32_t w = team.rank; w < node.mask_words; w += team.size) touched[w] = 0;
      // the right child, by the level's own distributor: x > val (binary_split.rs:52-57) or x != val (enumerate.rs:54-59)
      restrict_var(lv.x, (lv.w & kLevelEnum) ? (long long)(int)lv.y : (long long)bnd[lv.x].x, (long long)(int)lv.y);
      if constexpr (BNB) fold_bound();
      pending = lv.x;
    }
    node.end_node();
    if (last && team.leader()) atomicExch(a.stop, 1u);
    team.sync();
    if (last || (a.stop_on_solution && c_sols)) break;
  }
  if (reserved && team.leader()) atomicAdd(a.total_nodes, 0ull - (unsigned long long)reserved);  // what this tree reserved and did not run

  // ---- persist the tree: its current node, its stacks' lengths, its counters ---------------------------------------------------------------
  team.sync();
  copy_node(team, gbits, bits, V * sw);
  pcp_stats* const st_slot = a.stats + (blockIdx.x & (kStatSlots - 1));
  node.flush_stats(st_slot, c_nodes);
  if (team.leader()) {
    tree[0] = n_levels; tree[1] = misc[S_TRAILLEN]; tree[2] = pending; tree[3] = (finished ? 1u : 0u) | (min(given0, n_levels) << 8);
    unsigned long long* cn = a.counters + (size_t)t * 4;
    cn[0] += c_nodes; cn[1] += c_sols; cn[2] += c_fail;
    if (c_err) cn[3] = c_err;
    if (c_nodes) atomicAdd((unsigned long long*)&st_slot->nodes, c_nodes);
    if (c_fail) atomicAdd((unsigned long long*)&st_slot->failed_nodes, c_fail);
    if (c_err) atomicExch(a.stop, 1u);
  }
}

}  // namespace

}  // namespace pcp
