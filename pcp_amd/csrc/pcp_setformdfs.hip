// pcp_setformdfs.hip — the reference's search loop over FDSpace for stores that hold FORMULA propagators, on the device: the loop of
// setdfs_kernel (pcp_set.hip: the current node in LDS, an undo trail in HBM, Enumerate and branch and bound as template parameters) on the
// mapping of setformfix_kernel (pcp_setform.hip: one wavefront per node, one lane per formula unit).  gfx950.
//
// Formula stores are small — a node is a few hundred bytes of LDS — so a tree is ONE WAVEFRONT, not a 1024-thread workgroup: up to four
// trees per 256-thread workgroup, each on its own LDS slice, and a CU holds dozens of such chains (more chains per CU is the lever that
// helps search).  The trees of a workgroup are independent: there is no workgroup barrier anywhere in the kernel,
// a tree's steps are ordered by wave_sync (a workgroup-scope fence and a wave barrier) alone.
//   slice = setform_carve (bits[V][set_words], bnd[V], changed mask, unit live bits, 32 misc words) + `touched`, the variables a backtrack
//           restored and whose bounds it derives again.
// State, levels, trail and objective are setdfs_kernel's, byte for byte (pcp_forest_state, pcp_forest_objective; tree[4] = levels, trail
// length, pending, finished | given << 8; a level = (variable, value, trail mark, kLevelGiven | kLevelEnum); a trail entry = (word index,
// variable, removed bits lo, hi)), so setdfs_split_kernel, which reads no model table, hands work between these trees as it is.
//
// Per node: a chunked reservation from the forest's node counter (StopNode); Jacobi rounds over all LIVE units until a round narrows
// nothing — the unit step of pcp_setform.hpp on SetDomT<true>, every removal logged to the trail, the first step of a round deriving the
// bounds of the variables marked changed, an emptied set failing the node; the status of store.rs:250-256 (failed / no live unit: a
// solution / open); then the branch (FirstSmallestVar on cardinalities, the value and both children as setdfs_kernel under either
// distributor) or the backtrack (the trail ORed back down to the level's mark, the bounds of the touched variables, the right branch).
//
// Unit liveness is DERIVED, never stored with a node (DESIGN.md §2 "Implicit-active nodes" and "Formula units"): an entailed unit stays
// entailed as sets shrink, so a descent keeps the live bits; a backtrack widens sets, so it sets every unit live, and so does the start of
// a launch (a root, a persisted node, a node handed over by the split kernel) — the first round of that node unlinks again what is
// entailed, and running an entailed unit is a no-op (disjunction.rs:103), so the fixpoint and the status are the reference's either way.
//
// BNB: fold_bound as in setdfs_kernel — at launch start, after the branch restriction of a descent and of a backtrack; its trail entries
// lie above the level's mark, so a backtrack undoes them and the right child folds against the incumbent of that moment.
#include <algorithm>

#include "pcp_setform.hpp"

namespace pcp {

namespace {

struct SetFormDfsCarve { SetFormCarve c; size_t touched, total; };
__host__ __device__ inline SetFormDfsCarve setformdfs_carve(uint32_t V, uint32_t sw, uint32_t U) {
  SetFormDfsCarve d;
  d.c = setform_carve(V, sw, U);
  d.touched = d.c.total;
  d.total = (d.touched + ((size_t)(V + 31) / 32) * 4 + 15) & ~(size_t)15;
  return d;
}

template <bool ENUM, bool BNB>
__global__ void __launch_bounds__(256) setformdfs_kernel(const SetFormDfsArgs fa) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const SetDfsArgs& a = fa.d;
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6), nwv = blockDim.x >> 6;
  const uint32_t t = blockIdx.x * nwv + wv;
  if (t >= a.n_trees) return;  // (wave-uniform: the other trees of the workgroup never wait for this one)
  uint32_t* const tree = a.tree + (size_t)t * 4;
  if (__builtin_amdgcn_readfirstlane(tree[3]) & 1u) return;  // this tree is finished
  uint32_t n_levels = __builtin_amdgcn_readfirstlane(tree[0]), pending = __builtin_amdgcn_readfirstlane(tree[2]);
  const uint32_t given0 = __builtin_amdgcn_readfirstlane(tree[3]) >> 8;  // its oldest levels whose right branch went to another tree
  const uint32_t V = a.m.n_vars, sw = a.set_words, Wv = (V + 31) >> 5, U = fa.n_units, Wu = (U + 31) >> 5, nwords = V * sw;
  const SetFormDfsCarve dcv = setformdfs_carve(V, sw, U);
  unsigned char* const mine = smem + (size_t)wv * dcv.total;
  unsigned long long* const bits = reinterpret_cast<unsigned long long*>(mine + dcv.c.bits);
  int2* const bnd = reinterpret_cast<int2*>(mine + dcv.c.bnd);
  uint32_t* const chg = reinterpret_cast<uint32_t*>(mine + dcv.c.chg);
  uint32_t* const live = reinterpret_cast<uint32_t*>(mine + dcv.c.live);
  uint32_t* const misc = reinterpret_cast<uint32_t*>(mine + dcv.c.misc);
  uint32_t* const touched = reinterpret_cast<uint32_t*>(mine + dcv.touched);
  uint4* const trail = a.trail + (size_t)t * a.trail_cap;
  uint4* const levels = a.levels + (size_t)t * a.level_cap;
  unsigned long long* const gbits = reinterpret_cast<unsigned long long*>(a.bits) + (size_t)t * nwords;
  pcp_stats* const st_slot = a.stats + (blockIdx.x & (kStatSlots - 1));
  auto wave_sync = [] { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier(); };
  auto all_units_live = [&] {
    for (uint32_t w = lane; w < Wu; w += 64) live[w] = (w == Wu - 1 && (U & 31u)) ? (1u << (U & 31u)) - 1u : 0xFFFFFFFFu;
  };

  uint32_t narrow = 0, steps2 = 0, steps3 = 0;
  unsigned long long c_nodes = 0, c_sols = 0, c_fail = 0, c_rounds = 0;
  uint32_t c_err = 0;
  bool finished = false;
  uint32_t reserved = 0;       // nodes this tree may still run before it asks the forest's counter again
  bool res_has_last = false;   // ... the last of which is the node that reaches the limit
  using DM = SetDomT<true>;
  const DM dm{bits, bnd, a.m.const_val, V, sw, a.base, chg, misc, &narrow, trail, &misc[S_TRAILLEN], a.trail_cap};

  // a branch constraint folded into the variable's set: the values lo..hi leave it, one lane per word, every removal trailed
  auto restrict_var = [&](uint32_t var, long long lo, long long hi) {
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
    const long long best = (long long)__hip_atomic_load(a.obj_best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (a.obj_mode == PCP_MINIMIZE) restrict_var(a.obj_var, best, 1ll << 40);
    else restrict_var(a.obj_var, -(1ll << 40), best);
  };

  // ---- the tree's current node into its slice; every unit live; under BNB the incumbent of now; the bounds of every variable -----------
  if (lane < 32u) misc[lane] = 0;
  for (uint32_t w = lane; w < Wv; w += 64) { chg[w] = 0; touched[w] = 0; }
  all_units_live();
  for (uint32_t i = lane; i < nwords; i += 64) bits[i] = gbits[i];
  wave_sync();
  if (lane == 0) misc[S_TRAILLEN] = tree[1];
  wave_sync();
  if constexpr (BNB) { fold_bound(); wave_sync(); }
  {
    bool bad = false;
    for (uint32_t v = lane; v < V; v += 64) {
      const int2 b = scan_bounds(bits + (size_t)v * sw, sw, a.base);
      bnd[v] = b;
      bad |= b.x > b.y;  // an empty domain (a root's, or the objective's after the fold): the node fails
    }
    if (__ballot(bad) && lane == 0) misc[S_FAIL] = 1u;
    for (uint32_t w = lane; w < Wv; w += 64) chg[w] = 0;  // (the fold's mark: the bounds are exact)
  }
  wave_sync();

  for (uint32_t step = 0; step < a.n_steps; ++step) {
    // ---- may this node run?  The stop flag of the forest and the node limit of all trees together (StopNode, stop_node.rs:57-62): nodes
    // are reserved kDfsChunk at a time by lane 0; what a tree does not use goes back when the launch ends.  The node that reaches the limit
    // is explored and counted, but its status is replaced by EndOfSearch: it is neither a solution nor a failure.
    if (reserved == 0) {
      uint32_t got = 0, has_last = 0;
      if (lane == 0 && !__hip_atomic_load(a.stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
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
      reserved = __shfl(got, 0);
      res_has_last = __shfl(has_last, 0) != 0;
      if (!reserved) break;
    }
    --reserved;
    const bool last = res_has_last && reserved == 0;

    // ---- propagate: rounds over the live units until one narrows nothing ------------------------------------------------------------------
    bool failed = __builtin_amdgcn_readfirstlane(misc[S_FAIL]) != 0, runaway = false;
    uint32_t rounds = 0;
    while (!failed) {
      if (++rounds > (1u << 22)) { runaway = true; break; }  // (a round that is followed by another narrowed something: the cap only makes a runaway impossible)
      // the exact bounds of every variable marked changed — by the branch, the fold or the round before —, from its words
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
      const uint32_t before = narrow;
      for (uint32_t u = lane; u < U; u += 64) {
        if (!((live[u >> 5] >> (u & 31u)) & 1u)) continue;
        if (setform_unit_step(fa.nodes, fa.unit_root, a.m.recs, u, dm, steps2, steps3))
          atomicAnd(&live[u >> 5], ~(1u << (u & 31u)));  // unlink_prop (store.rs:200-207)
      }
      wave_sync();
      failed = __builtin_amdgcn_readfirstlane(misc[S_FAIL]) != 0;
      if (!__ballot(narrow != before)) break;
    }
    c_rounds += rounds;

    // ---- status (store.rs:250-256): failed / no subscription left: a solution / open ------------------------------------------------------
    bool any_live = false;
    for (uint32_t w = lane; w < Wu; w += 64) any_live |= live[w] != 0;
    const bool open = __ballot(any_live) != 0;
    const uint32_t tlen = __builtin_amdgcn_readfirstlane(misc[S_TRAILLEN]);
    if (__builtin_amdgcn_readfirstlane(misc[S_TRAILOVF])) { c_err = 4; break; }  // the trail is full: the tree cannot be restored any more (terminal)
    if (runaway) { c_err = 5; break; }
    ++c_nodes;
    bool descend = false;
    if (failed) {
      if (!last) ++c_fail;
    } else if (!open && last) {
    } else if (!open) {  // a solution (monitor.rs:19-68)
      ++c_sols;
      if constexpr (BNB) {
        // the incumbent is var.lower() in both modes (branch_and_bound.rs:73-77): the tree keeps the value and the row, then lowers / raises
        // the forest's incumbent (another tree may hold a better one already)
        const int v = bnd[a.obj_var].x;
        if (a.tree_row)
          for (uint32_t u = lane; u < V; u += 64) a.tree_row[(size_t)t * V + u] = bnd[u].x;
        if (lane == 0) {
          a.tree_best[t] = v;
          // (the old value is used, so the atomic has been performed before the backtrack below reads the incumbent for its fold)
          const int old = a.obj_mode == PCP_MINIMIZE ? __hip_atomic_fetch_min(a.obj_best, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                                     : __hip_atomic_fetch_max(a.obj_best, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          misc[S_CTL + 1] = (uint32_t)old;
        }
      } else if (a.first_solution) {  // the first one of the forest is kept
        uint32_t won = 0;
        if (lane == 0) won = atomicCAS(a.solution_flag, 0u, 1u) == 0u ? 1u : 0u;
        if (__shfl(won, 0))
          for (uint32_t v = lane; v < V; v += 64) a.first_solution[v] = bnd[v].x;
      }
      if (a.stop_on_solution && lane == 0) atomicExch(a.stop, 1u);
    } else {
      // Brancher<FirstSmallestVar, MiddleVal | MinVal, BinarySplit | Enumerate>::enter on sets: the variable of minimal CARDINALITY > 1,
      // first index (first_smallest_var.rs:30-39 on Domain::size()) — a popcount per variable, a minimum over the key size << 32 | v
      unsigned long long key = ~0ull;
      for (uint32_t v = lane; v < V; v += 64) {
        unsigned long long size = 0;
        for (uint32_t k = 0; k < sw; ++k) size += (unsigned long long)__popcll(bits[(size_t)v * sw + k]);
        if (size > 1) key = min(key, (size << 32) | v);
      }
      for (int o = 32; o > 0; o >>= 1) key = min(key, (unsigned long long)__shfl_xor(key, o));
      if (key == ~0ull) { c_err = 3; --c_nodes; if (lane == 0) atomicAdd(a.total_nodes, ~0ull); break; }  // Unknown, yet nothing to branch on: the reference panics
      if (n_levels >= a.level_cap) { c_err = 1; --c_nodes; pending = kDfsFull; if (lane == 0) atomicAdd(a.total_nodes, ~0ull); break; }
      const uint32_t var = (uint32_t)key;
      const int2 d = bnd[var];
      if constexpr (ENUM) {
        // MinVal: lower() (min_val.rs:25-27), a member; MiddleVal: (lower + upper) / 2 (middle_val.rs:25-27) or, when that is a hole of the
        // set, the member nearest to it, the lower one first: one lane per word, a minimum across the lanes
        long long v = d.x;
        if (a.val_mode != PCP_VAL_MIN) {
          const long long m = ((long long)d.x + (long long)d.y) / 2;
          unsigned long long nk = ~0ull;
          for (uint32_t k = lane; k < sw; k += 64) nk = min(nk, nearest_member_key(bits[(size_t)var * sw + k], (long long)a.base + 64ll * (long long)k, m));
          for (int o = 32; o > 0; o >>= 1) nk = min(nk, (unsigned long long)__shfl_xor(nk, o));
          v = nearest_member_value(nk, m);
        }
        if (lane == 0) levels[n_levels] = make_uint4(var, (uint32_t)(int)v, tlen, kLevelEnum);
        // the left child x = v (enumerate.rs:47-53): everything below v and everything above it leaves the set
        restrict_var(var, d.x, v - 1);
        restrict_var(var, v + 1, d.y);
      } else {
        const int val = (int)(((long long)d.x + (long long)d.y) / 2);  // MiddleVal (middle_val.rs:25-27)
        if (lane == 0) levels[n_levels] = make_uint4(var, (uint32_t)val, tlen, 0u);
        restrict_var(var, (long long)val + 1, d.y);  // the left child x <= val (binary_split.rs:46-57)
      }
      if constexpr (BNB) fold_bound();
      ++n_levels;
      pending = var;
      descend = true;  // (the live bits stay: what is entailed here is entailed below)
    }
    if (!descend) {
      // ---- backtrack: the deepest level whose right branch is still open (a level whose right branch was given to another tree is undone
      // like any other and skipped) ----------------------------------------------------------------------------------------------------------
      wave_sync();  // (this wavefront's trail and level entries, written by other lanes)
      uint4 lv = make_uint4(0u, 0u, 0u, kLevelGiven);
      uint32_t from = tlen;
      while (n_levels) {
        --n_levels;
        const uint4 q = levels[n_levels];
        lv = make_uint4(__builtin_amdgcn_readfirstlane(q.x), __builtin_amdgcn_readfirstlane(q.y), __builtin_amdgcn_readfirstlane(q.z), __builtin_amdgcn_readfirstlane(q.w));
        for (uint32_t i = lv.z + lane; i < from; i += 64) {
          const uint4 e = trail[i];
          atomicOr(&bits[e.x], ((unsigned long long)e.w << 32) | e.z);
          atomicOr(&touched[e.y >> 5], 1u << (e.y & 31u));
        }
        from = lv.z;
        if (!(lv.w & kLevelGiven)) break;
      }
      if (lv.w & kLevelGiven) { finished = true; break; }  // nothing left that is this tree's
      wave_sync();
      if (lane == 0) { misc[S_TRAILLEN] = from; misc[S_FAIL] = 0; }
      for (uint32_t v = lane; v < V; v += 64)
        if ((touched[v >> 5] >> (v & 31u)) & 1u) bnd[v] = scan_bounds(bits + (size_t)v * sw, sw, a.base);
      for (uint32_t w = lane; w < Wv; w += 64) chg[w] = 0;  // (a failed node leaves marks behind; every narrowed variable is a touched one)
      all_units_live();                                      // the sets grew: what was entailed below need not be here
      wave_sync();
      for (uint32_t w = lane; w < Wv; w += 64) touched[w] = 0;
      // the right child, by the level's own distributor: x > val (binary_split.rs:52-57) or x != val (enumerate.rs:54-59)
      restrict_var(lv.x, (lv.w & kLevelEnum) ? (long long)(int)lv.y : (long long)bnd[lv.x].x, (long long)(int)lv.y);
      if constexpr (BNB) fold_bound();
      pending = lv.x;
    }
    if (last && lane == 0) atomicExch(a.stop, 1u);
    wave_sync();
    if (last || (a.stop_on_solution && c_sols)) break;
  }
  if (reserved && lane == 0) atomicAdd(a.total_nodes, 0ull - (unsigned long long)reserved);  // what this tree reserved and did not run

  // ---- persist the tree: its current node, its stacks' lengths, its counters ---------------------------------------------------------------
  wave_sync();
  for (uint32_t i = lane; i < nwords; i += 64) gbits[i] = bits[i];
  for (int o = 32; o > 0; o >>= 1) { narrow += __shfl_down(narrow, o); steps2 += __shfl_down(steps2, o); steps3 += __shfl_down(steps3, o); }
  if (lane == 0) {
    tree[0] = n_levels; tree[1] = misc[S_TRAILLEN]; tree[2] = pending; tree[3] = (finished ? 1u : 0u) | (min(given0, n_levels) << 8);
    unsigned long long* cn = a.counters + (size_t)t * 4;
    cn[0] += c_nodes; cn[1] += c_sols; cn[2] += c_fail;
    if (c_err) cn[3] = c_err;
    const unsigned long long ev = (unsigned long long)steps2 + steps3;
    if (steps2) atomicAdd((unsigned long long*)&st_slot->steps, (unsigned long long)steps2);
    if (steps3) atomicAdd((unsigned long long*)&st_slot->steps3, (unsigned long long)steps3);
    if (ev) { atomicAdd((unsigned long long*)&st_slot->evaluated, ev); atomicAdd((unsigned long long*)&st_slot->full_evals, ev); }
    if (narrow) atomicAdd((unsigned long long*)&st_slot->narrowings, (unsigned long long)narrow);
    if (c_rounds) atomicAdd((unsigned long long*)&st_slot->waves, c_rounds);
    if (c_nodes) atomicAdd((unsigned long long*)&st_slot->nodes, c_nodes);
    if (c_fail) atomicAdd((unsigned long long*)&st_slot->failed_nodes, c_fail);
    if (c_err) atomicExch(a.stop, 1u);
  }
}

template <bool ENUM, bool BNB>
hipError_t launch_setformdfs_as(const SetFormDfsArgs& a, const LaunchPlan& p, hipStream_t stream) {
  hipError_t e;
  if (p.lds_bytes > 64 * 1024 &&
      (e = hipFuncSetAttribute(reinterpret_cast<const void*>(setformdfs_kernel<ENUM, BNB>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes)) != hipSuccess)
    return e;
  hipLaunchKernelGGL((setformdfs_kernel<ENUM, BNB>), dim3(p.grid), dim3(p.block), p.lds_bytes, stream, a);
  return hipGetLastError();
}

}  // namespace

size_t lds_bytes_setformdfs(uint32_t n_vars, uint32_t set_words, uint32_t n_units, uint32_t waves) {
  const SetFormDfsCarve c = setformdfs_carve(n_vars, set_words, n_units);
  return c.total * waves <= 160 * 1024 ? c.total * waves : 0;
}

// p.block = 64 x the trees of a workgroup, p.grid = ceil(n_trees / those), p.lds_bytes = lds_bytes_setformdfs of them
hipError_t launch_setformdfs(const SetFormDfsArgs& a, bool enumerate, bool bnb, const LaunchPlan& p, hipStream_t stream) {
  if (bnb) return enumerate ? launch_setformdfs_as<true, true>(a, p, stream) : launch_setformdfs_as<false, true>(a, p, stream);
  return enumerate ? launch_setformdfs_as<true, false>(a, p, stream) : launch_setformdfs_as<false, false>(a, p, stream);
}

}  // namespace pcp
