// pcp_formdfs.hip — the search loop over Interval<i32> stores that hold FORMULA propagators, on the device: row_dfs (pcp_rowdfs.hpp: the
// loop, its state and what a caller sees between two launches) with formfix_kernel's unit step as the propagation.  gfx950.
// This is the forest the scheduling models live in: propagators::Cumulative::join (propagators/cumulative.rs:59-114) allocates equivalences
// over Boolean, XEqYMulZ and Sum views, which set mode refuses.
//
// MI355X mapping: a formula store is small — a node is a few hundred bytes of LDS — so a tree is ONE WAVEFRONT, up to four trees per
// 256-thread workgroup, each on its own LDS slice (form_carve, the slice of formfix_kernel: nothing more is needed, the loop's own state is
// wave-uniform and sits in registers).  A tree is a latency chain; a CU wants as many chains as its registers allow.
// There is no workgroup barrier: the trees of a workgroup never wait for each other.
//
// ENUM = true (pcp_dfs_forest_device_form_enum): the loop under Enumerate.  The exclusion path, the rows' two words and the value re-choice
// are the loop's (pcp_rowdfs.hpp); this node runs the loop's sweep at the top of every round, fenced from the units that read what it
// wrote — formexcl_kernel's round (pcp_formexcl.hip) — and lends it the per-lane step count and F_OOB.  No LDS is added: the path and the
// rows' words are in HBM, the length of the current list is a wave-uniform register.  Unit liveness stays derived: the sweep never
// touches `live`, and an open exclusion keeps a node Unknown through the loop's ex_open.
#include <algorithm>
#include <type_traits>

#include "pcp_formula.hpp"
#include "pcp_rowdfs.hpp"

namespace pcp {

namespace {

// A node of formula units in its wavefront's slice: Jacobi rounds over the live units, a unit unlinked inside the round that finds it
// entailed, so that what is left of `live` after the rounds is what is still subscribed.
struct FormulaNode {
  enum : uint32_t { FAIL = F_FAIL, OOB = F_OOB, WORDS = F_WORDS };
  const FormDfsArgs& a;
  const uint32_t lane, V, S, U;
  const int32_t* const const_val;
  int2* dom;
  uint32_t *chg, *live, *misc;
  uint32_t steps2 = 0, steps3 = 0, acc_rounds = 0, acc_nodes = 0;  // (per lane resp. uniform; reduced and flushed once)
  Ctr& ctr;  // (the kernel's: a node whose `dm` pointed into the node itself could not be split into registers — it would live in scratch memory)
  const LdsDom dm;

  __device__ __forceinline__ FormulaNode(const FormDfsArgs& a_, unsigned char* mine, const FormCarve& cv, Ctr& ctr_)
      : a(a_), lane(threadIdx.x & 63), V(a_.m.n_vars), S(a_.m.n_slots), U(a_.n_units), const_val(a_.m.const_val),
        dom(reinterpret_cast<int2*>(mine + cv.dom)), chg(reinterpret_cast<uint32_t*>(mine + cv.chg)), live(reinterpret_cast<uint32_t*>(mine + cv.live)),
        misc(reinterpret_cast<uint32_t*>(mine + cv.misc)), ctr(ctr_), dm{dom, 1u, chg, &misc[F_FAIL], 1u, &ctr_, a_.m.sums} {}

  template <class Sweep>
  __device__ __forceinline__ bool propagate(bool failed, Sweep&& sweep) {
    uint32_t rounds = 0;
    while (!failed) {
      ++rounds;
      const uint32_t before = ctr.narrow;
      // the node's exclusions, then every live unit: formexcl_kernel's round (pcp_formexcl.hip).  The sweep writes `dom` through `dm`, the
      // units read it.  BinarySplit's callable is an empty type: nothing to run, no fence
      if constexpr (!std::is_empty_v<std::remove_reference_t<Sweep>>) { sweep(steps2); wave_sync(); }
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
    return failed;
  }
  __device__ __forceinline__ bool any_live(bool) const {
    bool any = false;
    for (uint32_t w = lane; w < ((U + 31) >> 5); w += 64) any |= live[w] != 0;
    return any;
  }
  __device__ __forceinline__ void flush_stats(pcp_stats* stats) const { flush_node_stats(stats, lane, steps2, steps3, ctr.narrow, acc_rounds, acc_nodes); }
};

template <bool BNB, bool ENUM, bool SINK, bool INPUT_ORDER>
__global__ void __launch_bounds__(256) formdfs_kernel(const FormDfsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nwv = blockDim.x >> 6;
  const FormCarve cv = form_carve(a.m.n_slots, a.n_units);
  Ctr ctr;
  FormulaNode node(a, smem + (size_t)wv * cv.total, cv, ctr);
  row_dfs<BNB, ENUM, SINK, INPUT_ORDER>(a.d, blockIdx.x * nwv + wv, node);
}

template <bool BNB, bool ENUM, bool SINK, bool INPUT_ORDER>
hipError_t launch_formdfs_io(const FormDfsArgs& a, const LaunchPlan& p, hipStream_t stream) {
  hipError_t e;
  if (p.lds_bytes > 64 * 1024 &&
      (e = hipFuncSetAttribute(reinterpret_cast<const void*>(formdfs_kernel<BNB, ENUM, SINK, INPUT_ORDER>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes)) != hipSuccess)
    return e;
  hipLaunchKernelGGL((formdfs_kernel<BNB, ENUM, SINK, INPUT_ORDER>), dim3(p.grid), dim3(p.block), p.lds_bytes, stream, a);
  return hipGetLastError();
}

// The variable selector (option "var_select", a.d.var_select) is a template flag here, not a run-time mask on the key as in the other
// branchers: these kernels have no scalar register to spare (over 100 SGPR spills each), and one more live scalar moved the default path's
// spills — up to 2.5 % on the small-store forest (profiles/var_select_measured.jsonl).  FirstSmallestVar's instantiations are the code
// they were.
template <bool BNB, bool ENUM, bool SINK>
hipError_t launch_formdfs_as(const FormDfsArgs& a, const LaunchPlan& p, hipStream_t stream) {
  return a.d.var_select == PCP_VAR_INPUT_ORDER ? launch_formdfs_io<BNB, ENUM, SINK, true>(a, p, stream) : launch_formdfs_io<BNB, ENUM, SINK, false>(a, p, stream);
}

}  // namespace

size_t lds_bytes_formdfs(uint32_t n_slots, uint32_t n_units, uint32_t waves) {
  const FormCarve c = form_carve(n_slots, n_units);
  return c.total * waves <= 160 * 1024 ? c.total * waves : 0;
}

// p.block = 64 x the trees of a workgroup, p.grid = ceil(n_trees / those), p.lds_bytes = lds_bytes_formdfs of them
hipError_t launch_formdfs(const FormDfsArgs& a, bool bnb, const LaunchPlan& p, hipStream_t stream) {
  // the context's solution sink (pcp_solution_sink_set); the branch-and-bound entries refuse it
  const bool sink = a.d.sink.lb != nullptr;
  if (sink && (bnb || !a.d.sink.ub || !a.d.sink.count || !a.d.sink.capacity)) return hipErrorInvalidValue;
  if (a.d.row_base) {  // Enumerate: the rows' words are there (pcp_dfs_forest_device_form_enum)
    if (!a.d.row_excl || (a.d.path_capacity && !a.d.path)) return hipErrorInvalidValue;
    if (sink) return launch_formdfs_as<false, true, true>(a, p, stream);
    return bnb ? launch_formdfs_as<true, true, false>(a, p, stream) : launch_formdfs_as<false, true, false>(a, p, stream);
  }
  if (sink) return launch_formdfs_as<false, false, true>(a, p, stream);
  return bnb ? launch_formdfs_as<true, false, false>(a, p, stream) : launch_formdfs_as<false, false, false>(a, p, stream);
}

}  // namespace pcp
