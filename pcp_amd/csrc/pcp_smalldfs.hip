// pcp_smalldfs.hip — the search loop over SMALL Interval<i32> stores of plain propagators, on the device: row_dfs (pcp_rowdfs.hpp: the loop,
// its state and what a caller sees between two launches) with smallfix_kernel's round as the propagation.  gfx950.
// These are the stores smallfix_kernel propagates (pcp_small.hip, plan.path 4): at most 128 slots and 2048 elementary filters, no formula
// units — Distinct, XLessY, XEqY, XEqYPlusZ, XLessYPlusZ, XGreaterYPlusZ, XEqYMulZ and Sum views in any mixture; BASELINE config 4, the
// Golomb-ruler network, is one of them, and the only optimisation benchmark of the project.
//
// MI355X mapping: that of formdfs_kernel (pcp_formdfs.hip) — a tree is ONE WAVEFRONT, up to four trees per 256-thread workgroup, each on
// its own LDS slice, the loop's own state wave-uniform in registers — with smallfix_kernel's round as the propagation step
// (pcp_small.hpp: the all-different units through their 128-value mask, then every record of a live unit, lane-strided).  The records
// come from ONE LDS copy per workgroup, made once per launch by all its wavefronts and published by the kernel's only __syncthreads();
// every wavefront reaches that barrier — a workgroup with three trees, or with a finished one, leaves nobody behind it — and only then
// enters row_dfs, which takes the wave-uniform exits.  After it the trees of a workgroup never wait for each other.
//
// ENUM = true (pcp_dfs_forest_device_small_enum): the loop under Enumerate.  The invariant it rests on — every open row's exclusion list is
// a prefix of the current path plus at most one entry of its own — and the path sweep are the loop's (pcp_rowdfs.hpp); this node only
// runs the sweep where smallfix_kernel runs a node's own units, at the top of a round, and lends it the round's step count and S_OOB.
#include <algorithm>

#include "pcp_rowdfs.hpp"
#include "pcp_small.hpp"

namespace pcp {

namespace {

// A node of plain propagators in its wavefront's slice: smallfix_kernel's rounds over the live units; the round that narrows nothing
// leaves in `ent` the entailment on the final domains, and any_live unlinks by it.
struct SmallNode {
  enum : uint32_t { FAIL = S_FAIL, OOB = S_OOB, WORDS = S_WORDS };
  const SmallShared& sh;
  const SmallSlice sl;
  const uint32_t lane, V, S, U, P;
  const int32_t* const const_val;
  int2* const dom;
  uint32_t *const chg, *const live, *const misc;
  unsigned long long steps2 = 0, steps3 = 0;  // (per lane; reduced and flushed once)
  uint32_t acc_rounds = 0, acc_nodes = 0;
  Ctr& ctr;  // (the kernel's: a node whose `dm` pointed into the node itself could not be split into registers — it would live in scratch memory)
  const LdsDom dm;

  __device__ __forceinline__ SmallNode(const SmallDfsArgs& a, const SmallShared& sh_, const SmallSlice& sl_, Ctr& ctr_)
      : sh(sh_), sl(sl_), lane(threadIdx.x & 63), V(a.m.n_vars), S(a.m.n_slots), U(a.n_units), P(a.m.n_recs), const_val(a.m.const_val),
        dom(sl_.dom), chg(sl_.chg), live(sl_.live), misc(sl_.misc), ctr(ctr_), dm{dom, 1u, chg, &misc[S_FAIL], 1u, &ctr_, a.m.sums} {}

  template <class Sweep>
  __device__ __forceinline__ bool propagate(bool failed, Sweep&& sweep) {
    uint32_t rounds = 0, s2 = 0, s3 = 0;
    while (!failed) {
      ++rounds;
      const uint32_t before = ctr.narrow;
      small_round(sh, P, (U + 31) >> 5, sl, dm, lane, s2, s3, [&] { sweep(s2); });
      small_wave_sync();
      failed = __builtin_amdgcn_readfirstlane(misc[S_FAIL]) != 0;
      if (!__ballot(ctr.narrow != before)) break;
    }
    steps2 += s2; steps3 += s3;
    acc_rounds += rounds ? rounds : 1;
    ++acc_nodes;
    return failed;
  }
  // unlink_prop (store.rs:200-207): the last round narrowed nothing, so its `ent` is the entailment on the final domains
  __device__ __forceinline__ bool any_live(bool failed) const {
    bool any = false;
    if (!failed)
      for (uint32_t w = lane; w < ((U + 31) >> 5); w += 64) {
        const uint32_t left = live[w] & ~sl.ent[w];
        live[w] = left;
        any |= left != 0;
      }
    return any;
  }
  __device__ __forceinline__ void flush_stats(pcp_stats* stats) const { flush_node_stats(stats, lane, steps2, steps3, ctr.narrow, acc_rounds, acc_nodes); }
};

template <bool BNB, bool ENUM, bool SINK, bool INPUT_ORDER>
__global__ void __launch_bounds__(256) smalldfs_kernel(const SmallDfsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nwv = blockDim.x >> 6;
  // the records, once per launch, by every wavefront of the workgroup — also those that have no tree to run: the barrier stands ahead of
  // every wave-uniform exit of row_dfs
  const SmallShared sh = small_copy_shared(smem, a.m.n_recs, a.m.recs, a.rec_unit, a.ad_tab, a.ad_vars);
  __syncthreads();
  Ctr ctr;
  SmallNode node(a, sh, small_slice(smem, a.m.n_recs, a.m.n_slots, a.n_units, wv), ctr);
  row_dfs<BNB, ENUM, SINK, INPUT_ORDER>(a.d, blockIdx.x * nwv + wv, node);
}

template <bool BNB, bool ENUM, bool SINK, bool INPUT_ORDER>
hipError_t launch_smalldfs_io(const SmallDfsArgs& a, const LaunchPlan& p, hipStream_t stream) {
  hipError_t e;
  if (p.lds_bytes > 64 * 1024 &&
      (e = hipFuncSetAttribute(reinterpret_cast<const void*>(smalldfs_kernel<BNB, ENUM, SINK, INPUT_ORDER>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes)) != hipSuccess)
    return e;
  hipLaunchKernelGGL((smalldfs_kernel<BNB, ENUM, SINK, INPUT_ORDER>), dim3(p.grid), dim3(p.block), p.lds_bytes, stream, a);
  return hipGetLastError();
}

// The variable selector (option "var_select", a.d.var_select) is a template flag here, not a run-time mask on the key as in the other
// branchers: these kernels have no scalar register to spare (over 100 SGPR spills each), and one more live scalar moved the default path's
// spills — up to 2.5 % on the small-store forest (profiles/var_select_measured.jsonl).  FirstSmallestVar's instantiations are the code
// they were.
template <bool BNB, bool ENUM, bool SINK>
hipError_t launch_smalldfs_as(const SmallDfsArgs& a, const LaunchPlan& p, hipStream_t stream) {
  return a.d.var_select == PCP_VAR_INPUT_ORDER ? launch_smalldfs_io<BNB, ENUM, SINK, true>(a, p, stream) : launch_smalldfs_io<BNB, ENUM, SINK, false>(a, p, stream);
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
  const bool sink = a.d.sink.lb != nullptr;
  if (sink && (bnb || !a.d.sink.ub || !a.d.sink.count || !a.d.sink.capacity)) return hipErrorInvalidValue;
  if (a.d.row_base) {  // Enumerate: the rows' words are there (pcp_dfs_forest_device_small_enum)
    if (!a.d.row_excl || (a.d.path_capacity && !a.d.path)) return hipErrorInvalidValue;
    if (sink) return launch_smalldfs_as<false, true, true>(a, p, stream);
    return bnb ? launch_smalldfs_as<true, true, false>(a, p, stream) : launch_smalldfs_as<false, true, false>(a, p, stream);
  }
  if (sink) return launch_smalldfs_as<false, false, true>(a, p, stream);
  return bnb ? launch_smalldfs_as<true, false, false>(a, p, stream) : launch_smalldfs_as<false, false, false>(a, p, stream);
}

}  // namespace pcp
