// pcp_setformdfs.hip — the search loop over FDSpace for stores that hold FORMULA propagators, on the device: trail_dfs (pcp_setdfs.hpp: the
// loop, the trail, Enumerate and branch and bound) on the mapping of setformfix_kernel (pcp_setform.hip: one wavefront per node, one lane
// per formula unit).  gfx950.
//
// Formula stores are small — a node is a few hundred bytes of LDS — so a tree is ONE WAVEFRONT (WavefrontTeam), not a 1024-thread
// workgroup: up to four trees per 256-thread workgroup, each on its own LDS slice, and a CU holds dozens of such chains (more chains per
// CU is the lever that helps search).
//   slice = setform_carve (bits[V][set_words], bnd[V], changed mask, unit live bits, 32 misc words) + `touched`, the variables a backtrack
//           restored and whose bounds it derives again.
#include <algorithm>

#include "pcp_setdfs.hpp"
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

// A node of the formula forest: Jacobi rounds over all LIVE units until a round narrows nothing — the unit step of pcp_setform.hpp on
// SetDomT<true>, every removal logged to the trail, the first step of a round deriving the bounds of the variables marked changed, an
// emptied set failing the node.
//
// Unit liveness is DERIVED, never stored with a node (DESIGN.md §2 "Implicit-active nodes" and "Formula units"): an entailed unit stays
// entailed as sets shrink, so a descent keeps the live bits; a backtrack widens sets, so it sets every unit live, and so does the start of
// a launch (a root, a persisted node, a node handed over by the split kernel) — the first round of that node unlinks again what is
// entailed, and running an entailed unit is a no-op (disjunction.rs:103), so the fixpoint and the status are the reference's either way.
struct FormulaNode {
  using DM = SetDomT<true>;
  const SetFormDfsArgs& fa;
  const WavefrontTeam& team;
  unsigned long long* bits;
  int2* bnd;
  uint32_t *chg, *live, *misc, *touched;
  uint4* trail;
  uint32_t mask_words, unit_words;
  uint32_t narrow = 0, steps2 = 0, steps3 = 0;
  unsigned long long c_rounds = 0;
  bool failed = false;

  __device__ __forceinline__ FormulaNode(const SetFormDfsArgs& fa_, const WavefrontTeam& team_, unsigned char* mine, const SetFormDfsCarve& dcv, uint32_t t)
      : fa(fa_), team(team_),
        bits(reinterpret_cast<unsigned long long*>(mine + dcv.c.bits)), bnd(reinterpret_cast<int2*>(mine + dcv.c.bnd)),
        chg(reinterpret_cast<uint32_t*>(mine + dcv.c.chg)), live(reinterpret_cast<uint32_t*>(mine + dcv.c.live)),
        misc(reinterpret_cast<uint32_t*>(mine + dcv.c.misc)), touched(reinterpret_cast<uint32_t*>(mine + dcv.touched)),
        trail(fa_.d.trail + (size_t)t * fa_.d.trail_cap), mask_words((fa_.d.m.n_vars + 31) >> 5), unit_words((fa_.n_units + 31) >> 5) {}

  __device__ __forceinline__ uint32_t* mark_mask() const { return chg; }
  __device__ __forceinline__ void all_units_live() {
    const uint32_t U = fa.n_units;
    for (uint32_t w = team.lane; w < unit_words; w += 64) live[w] = (w == unit_words - 1 && (U & 31u)) ? (1u << (U & 31u)) - 1u : 0xFFFFFFFFu;
  }
  __device__ __forceinline__ void clear_marks() {
    for (uint32_t w = team.lane; w < mask_words; w += 64) chg[w] = 0;
  }

  __device__ __forceinline__ void load(const unsigned long long* gbits) {
    const uint32_t lane = team.lane;
    if (lane < 32u) misc[lane] = 0;
    for (uint32_t w = lane; w < mask_words; w += 64) { chg[w] = 0; touched[w] = 0; }
    all_units_live();
    copy_node(team, bits, gbits, fa.d.m.n_vars * fa.d.set_words);
    team.sync();
  }
  __device__ __forceinline__ void begin(uint32_t) { team.sync(); }  // (S_TRAILLEN, before the fold appends to the trail)
  // launch start, after the fold: the bounds of every variable
  __device__ __forceinline__ void begun() {
    const SetDfsArgs& a = fa.d;
    bool bad = false;
    for (uint32_t v = team.lane; v < a.m.n_vars; v += 64) {
      const int2 b = scan_bounds(bits + (size_t)v * a.set_words, a.set_words, a.base);
      bnd[v] = b;
      bad |= b.x > b.y;  // an empty domain (a root's, or the objective's after the fold): the node fails
    }
    if (__ballot(bad) && team.lane == 0) misc[S_FAIL] = 1u;
    clear_marks();  // (the fold's mark: the bounds are exact)
    team.sync();
  }

  // rounds over the live units until one narrows nothing
  __device__ __forceinline__ bool propagate(uint32_t) {
    const SetDfsArgs& a = fa.d;
    const uint32_t lane = team.lane, V = a.m.n_vars, sw = a.set_words, U = fa.n_units;
    const DM dm{bits, bnd, a.m.const_val, V, sw, a.base, chg, misc, &narrow, trail, &misc[S_TRAILLEN], a.trail_cap};
    failed = __builtin_amdgcn_readfirstlane(misc[S_FAIL]) != 0;
    bool runaway = false;
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
      team.sync();
      clear_marks();
      team.sync();
      if (__ballot(emptied)) { failed = true; break; }
      const uint32_t before = narrow;
      for (uint32_t u = lane; u < U; u += 64) {
        if (!((live[u >> 5] >> (u & 31u)) & 1u)) continue;
        if (setform_unit_step(fa.nodes, fa.unit_root, a.m.recs, u, dm, steps2, steps3))
          atomicAnd(&live[u >> 5], ~(1u << (u & 31u)));  // unlink_prop (store.rs:200-207)
      }
      team.sync();
      failed = __builtin_amdgcn_readfirstlane(misc[S_FAIL]) != 0;
      if (!__ballot(narrow != before)) break;
    }
    c_rounds += rounds;
    return runaway;
  }

  // status (store.rs:250-256): failed / no subscription left: a solution / open
  __device__ __forceinline__ NodeStatus status() {
    bool any_live = false;
    for (uint32_t w = team.lane; w < unit_words; w += 64) any_live |= live[w] != 0;
    const bool open = __ballot(any_live) != 0;
    return NodeStatus{failed, open};
  }
  // (a solution node does not pay for the key: only the branch asks for it)
  __device__ __forceinline__ unsigned long long branch_key() const { return first_smallest_var(team, bits, fa.d.m.n_vars, fa.d.set_words, fa.d.var_select); }
  __device__ __forceinline__ void backtracking() { team.sync(); }  // (this wavefront's trail and level entries, written by other lanes)
  __device__ __forceinline__ void backtracked() {
    clear_marks();     // (a failed node leaves marks behind; every narrowed variable is a touched one)
    all_units_live();  // the sets grew: what was entailed below need not be here
  }
  __device__ __forceinline__ void end_node() {}
  __device__ __forceinline__ void flush_stats(pcp_stats* st_slot, unsigned long long) {
    for (int o = 32; o > 0; o >>= 1) { narrow += __shfl_down(narrow, o); steps2 += __shfl_down(steps2, o); steps3 += __shfl_down(steps3, o); }
    if (team.lane == 0) {
      const unsigned long long ev = (unsigned long long)steps2 + steps3;
      if (steps2) atomicAdd((unsigned long long*)&st_slot->steps, (unsigned long long)steps2);
      if (steps3) atomicAdd((unsigned long long*)&st_slot->steps3, (unsigned long long)steps3);
      if (ev) { atomicAdd((unsigned long long*)&st_slot->evaluated, ev); atomicAdd((unsigned long long*)&st_slot->full_evals, ev); }
      if (narrow) atomicAdd((unsigned long long*)&st_slot->narrowings, (unsigned long long)narrow);
      if (c_rounds) atomicAdd((unsigned long long*)&st_slot->waves, c_rounds);
    }
  }
};

template <bool ENUM, bool BNB, bool SINK>
__global__ void __launch_bounds__(256) setformdfs_kernel(const SetFormDfsArgs fa, const SetSinkDev sink) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nwv = blockDim.x >> 6;
  const uint32_t t = blockIdx.x * nwv + wv;
  if (t >= fa.d.n_trees) return;  // (wave-uniform: the other trees of the workgroup never wait for this one)
  const SetFormDfsCarve dcv = setformdfs_carve(fa.d.m.n_vars, fa.d.set_words, fa.n_units);
  const WavefrontTeam team;
  FormulaNode node(fa, team, smem + (size_t)wv * dcv.total, dcv, t);
  trail_dfs<ENUM, BNB, SINK>(fa.d, sink, t, team, node);
}

template <bool ENUM, bool BNB, bool SINK>
hipError_t launch_setformdfs_as(const SetFormDfsArgs& a, const SetSinkDev& sink, const LaunchPlan& p, hipStream_t stream) {
  hipError_t e;
  if (p.lds_bytes > 64 * 1024 &&
      (e = hipFuncSetAttribute(reinterpret_cast<const void*>(setformdfs_kernel<ENUM, BNB, SINK>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes)) != hipSuccess)
    return e;
  hipLaunchKernelGGL((setformdfs_kernel<ENUM, BNB, SINK>), dim3(p.grid), dim3(p.block), p.lds_bytes, stream, a, sink);
  return hipGetLastError();
}

}  // namespace

size_t lds_bytes_setformdfs(uint32_t n_vars, uint32_t set_words, uint32_t n_units, uint32_t waves) {
  const SetFormDfsCarve c = setformdfs_carve(n_vars, set_words, n_units);
  return c.total * waves <= 160 * 1024 ? c.total * waves : 0;
}

// p.block = 64 x the trees of a workgroup, p.grid = ceil(n_trees / those), p.lds_bytes = lds_bytes_setformdfs of them
hipError_t launch_setformdfs(const SetFormDfsArgs& a, const SetSinkDev& sk, bool enumerate, bool bnb, const LaunchPlan& p, hipStream_t stream) {
  // the context's set solution sink (pcp_set_solution_sink_set); the branch-and-bound entry refuses it
  const bool sink = sk.bits != nullptr;
  if (sink && (bnb || !sk.count || !sk.capacity)) return hipErrorInvalidValue;
  if (bnb) return enumerate ? launch_setformdfs_as<true, true, false>(a, sk, p, stream) : launch_setformdfs_as<false, true, false>(a, sk, p, stream);
  if (sink) return enumerate ? launch_setformdfs_as<true, false, true>(a, sk, p, stream) : launch_setformdfs_as<false, false, true>(a, sk, p, stream);
  return enumerate ? launch_setformdfs_as<true, false, false>(a, sk, p, stream) : launch_setformdfs_as<false, false, false>(a, sk, p, stream);
}

}  // namespace pcp
