// pcp_setform.hip — the propagation fixpoint of stores that hold FORMULA propagators (the reified layer, logic/) over IntervalSet<i32>
// domains: pcp_formula.hip's trees of Conjunction / Disjunction nodes over elementary leaves, evaluated on pcp_set.hip's bit sets.  gfx950.
//
// The reference's reified layer is generic in the domain (logic/*.rs are written against the Subsumption / Propagator traits only), and its
// default space FDSpace holds IntervalSet domains (variable/mod.rs:38, search/mod.rs:41-43): over sets a leaf's is_subsumed() sees more than
// over intervals — XEqY is disentailed as soon as the two SETS are disjoint, whatever their hulls (x_eq_y.rs:87-93 through
// IntervalSet::is_disjoint) — so a Disjunction unit-propagates earlier and the fixpoints differ from interval mode's.
//
// MI355X mapping, as formfix_kernel: one WAVEFRONT per node, up to four per workgroup, persistent workgroups; one lane per unit
// (lane-strided beyond 64 units); a unit's tree walked by two loops over its breadth-first node array with 64-bit true / false / active
// masks; rounds until a round narrows nothing.  The node lives in the wavefront's LDS slice as in setfix_kernel:
//   bits[V][set_words] u64   value v of variable x <-> bit (v - base) of bits[x]; narrowing = ds_and_b64 (SetDomT, pcp_setdom.hpp)
//   bnd[V] (lb, ub)          the sets' bounds, re-derived at the start of a round for the variables the round before marked changed
// Parity with the reference's FIFO (DESIGN.md §2 "Formula units" and "Set mode"): the filters are monotone and contracting;
// is_subsumed() only moves from Unknown to True or False as sets shrink, so a decision taken on an older set is the conservative one and
// the next round repeats it; between two bounds steps a cached bound is a superset read.  The last round narrows nothing, so it has seen
// exact bounds and final sets throughout.
// These stores are small and branchy: the kernel is written for correctness and occupancy of the chip by nodes, not for bandwidth.
#include <algorithm>

#include "pcp_neq.h"
#include "pcp_setdom.hpp"

namespace pcp {

namespace {

struct SetFormCarve {
  size_t bits, bnd, chg, live, misc, total;
};
__host__ __device__ inline SetFormCarve setform_carve(uint32_t V, uint32_t sw, uint32_t U) {
  auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
  SetFormCarve c;
  size_t o = 0;
  c.bits = o; o = up(o + (size_t)V * sw * 8);
  c.bnd = o; o = up(o + (size_t)V * 8);
  c.chg = o; o = up(o + (size_t)((V + 31) / 32) * 4);
  c.live = o; o = up(o + (size_t)((U + 31) / 32) * 4);
  c.misc = o; o = up(o + 32 * 4);  // the S_* words SetDomT names (S_FAIL; S_TRAILOVF is never written without a trail)
  c.total = o;
  return c;
}

__device__ __forceinline__ uint32_t kleene_and(uint32_t a, uint32_t b) { return (a == 0u || b == 0u) ? 0u : ((a == 1u && b == 1u) ? 1u : 2u); }
__device__ __forceinline__ uint32_t kleene_not(uint32_t a) { return a == 2u ? 2u : 1u - a; }

// is_subsumed() of one elementary propagator as SKleene (0 False, 1 True, 2 Unknown), on IntervalSet<i32> domains:
//   XEqY x_eq_y.rs:73-94 (False iff the SETS are disjoint) | XNeqY x_neq_y.rs:71-73 (not XEqY) | XLessY x_less_y.rs:73-95 |
//   XLessYPlusZ x_less_y_plus_z.rs:82-97 | XGreaterYPlusZ x_greater_y_plus_z.rs:82-98 | XEqYPlusZ x_eq_y_plus_z.rs:60-67 (Kleene and of
//   its halves) | Boolean boolean.rs:111-127 | BooleanNeg boolean_neg.rs:71-79.  A Constant operand is a singleton without words.
__device__ __forceinline__ uint32_t rec_subsumed_set(const Rec& rec, const SetDom& dm) {
  const uint32_t kind = rec.xk >> 28, x = rec.xk & kSlotMask;
  const long long d = rec.d;
  const int2 X = dm.bounds(x);
  if (X.x > X.y) return 2u;  // an emptied set: the node has failed (found by the next bounds step)
  if (kind == PCP_BOOL || kind == PCP_NBOOL) {  // the view is x + d; Boolean: singleton ? (value == 1) : Unknown
    uint32_t b = 2u;
    if (X.x == X.y) b = ((long long)X.x + d == 1) ? 1u : 0u;
    return kind == PCP_BOOL ? b : kleene_not(b);
  }
  const uint32_t y = rec.y;
  const int2 Y = dm.bounds(y);
  if (Y.x > Y.y) return 2u;
  if (kind <= PCP_LT) {
    const long long Yl = (long long)Y.x + d, Yu = (long long)Y.y + d;
    if (kind == PCP_LT) return X.x >= Yu ? 0u : (X.y < Yl ? 1u : 2u);
    uint32_t eq = 2u;
    if (X.x == Yu && X.y == Yl) eq = 1u;                                     // both singletons and equal
    else if (X.x > Yu || Yl > X.y) eq = 0u;                                  // the hulls are disjoint
    else if (X.x == X.y) eq = dm.test(y, (int)(X.x - d)) ? 2u : 0u;          // a singleton (a Constant is one): membership in the other set
    else if (Y.x == Y.y) eq = dm.test(x, (int)(Y.x + d)) ? 2u : 0u;
    else if (dm.disjoint_shifted(x, y, d)) eq = 0u;                          // two variables: the words
    return kind == PCP_EQ ? eq : kleene_not(eq);
  }
  const int2 Z = dm.bounds(rec.z);
  if (Z.x > Z.y) return 2u;
  auto lt3 = [&](long long dd) -> uint32_t {  // x < y + z + dd
    return (long long)X.x >= (long long)Y.y + Z.y + dd ? 0u : ((long long)X.y < (long long)Y.x + Z.x + dd ? 1u : 2u);
  };
  auto gt3 = [&](long long dd) -> uint32_t {  // x > y + z + dd
    return (long long)X.y <= (long long)Y.x + Z.x + dd ? 0u : ((long long)X.x > (long long)Y.y + Z.y + dd ? 1u : 2u);
  };
  if (kind == PCP_LT3) return lt3(d);
  if (kind == PCP_GT3) return gt3(d);
  if (kind == PCP_EQ3) return kleene_and(gt3(d - 1), lt3(d + 1));
  return 2u;  // XEqYMulZ on sets is rejected on the host (pcp_model_push_props / _push_formula)
}

// propagate() of one elementary leaf.  A failure raises the node's fail flag (every caller ends the node on it).
__device__ __forceinline__ void rec_propagate_set(const Rec& rec, const SetDom& dm) {
  const uint32_t kind = rec.xk >> 28;
  if (kind == PCP_BOOL || kind == PCP_NBOOL) {
    // Boolean::propagate = update(var, {1}) (boolean.rs:130-138); BooleanNeg: {0} (boolean_neg.rs:81-90): every other value is cleared
    // through SetDom.  A set without that value is a non-monotonic update — the reference panics (variable/store.rs:153-156); here the
    // node fails (pcp_hip.h).
    const uint32_t x = rec.xk & kSlotMask;
    const int want = (kind == PCP_BOOL ? 1 : 0) - rec.d;
    if (!dm.test(x, want)) { dm.fail(); return; }
    if (dm.is_const(x)) return;
    const int2 X = dm.bounds(x);
    if (X.x < want) dm.clear_range(x, X.x, (long long)want - 1);
    if (X.y > want) dm.clear_range(x, (long long)want + 1, X.y);
    return;
  }
  (void)eval_set(rec, dm, false);  // the filter half: propagate() of the six comparison kinds on sets
}

// See the head of the file.  IMPLICIT: no `active` rows are read, every unit starts live (liveness is derived: an entailed unit is unlinked
// in either mode — its propagate() is a no-op from then on, disjunction.rs:103); rows are written when active_out is given.
template <bool IMPLICIT>
__global__ void __launch_bounds__(256) setformfix_kernel(const SetFormArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6), nwv = blockDim.x >> 6;
  const uint32_t V = a.m.n_vars, sw = a.set_words, Wv = (V + 31) >> 5, U = a.n_units, Wu = (U + 31) >> 5;
  const SetFormCarve cv = setform_carve(V, sw, U);
  unsigned char* const mine = smem + (size_t)wv * cv.total;
  unsigned long long* const bits = reinterpret_cast<unsigned long long*>(mine + cv.bits);
  int2* const bnd = reinterpret_cast<int2*>(mine + cv.bnd);
  uint32_t* const chg = reinterpret_cast<uint32_t*>(mine + cv.chg);
  uint32_t* const live = reinterpret_cast<uint32_t*>(mine + cv.live);
  uint32_t* const misc = reinterpret_cast<uint32_t*>(mine + cv.misc);
  const uint32_t words64 = (U + 63) >> 6, nwords = V * sw;
  auto wave_sync = [] { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier(); };
  pcp_stats* const stats = a.stats + (blockIdx.x & (kStatSlots - 1));
  unsigned long long acc_s2 = 0, acc_s3 = 0, acc_narrow = 0, acc_waves = 0, acc_nodes = 0, acc_failed = 0;

  for (uint32_t node = blockIdx.x * nwv + wv; node < a.n_nodes; node += gridDim.x * nwv) {
    const size_t row = (size_t)node * V;
    if (lane < 32u) misc[lane] = 0;
    for (uint32_t w = lane; w < Wv; w += 64) chg[w] = 0;
    // Store::active (one bit per unit): the caller's row, or every unit
    for (uint32_t w = lane; w < Wu; w += 64) {
      uint32_t lv = 0xFFFFFFFFu;
      if constexpr (!IMPLICIT) {
        if (a.active_in) { const uint64_t q = a.active_in[(size_t)node * words64 + (w >> 1)]; lv = (uint32_t)(q >> (32 * (w & 1))); }
      }
      if (w == Wu - 1 && (U & 31u)) lv &= (1u << (U & 31u)) - 1u;
      live[w] = lv;
    }
    {
      const uint64_t* src = a.bits_in + row * sw;
      for (uint32_t i = lane; i < nwords; i += 64) bits[i] = src[i];
    }
    wave_sync();
    bool bad = false;
    for (uint32_t v = lane; v < V; v += 64) {
      const int2 b = scan_bounds(bits + (size_t)v * sw, sw, a.base);
      bnd[v] = b;
      bad |= b.x > b.y;  // an empty input domain
    }
    if (__ballot(bad) && lane == 0) misc[S_FAIL] = 1u;
    wave_sync();

    uint32_t narrow = 0, steps2 = 0, steps3 = 0, rounds = 0;
    const SetDom dm{bits, bnd, a.m.const_val, V, sw, a.base, chg, misc, &narrow};
    auto leaf_propagate = [&](const Rec& rec) {
      const uint32_t kind = rec.xk >> 28;
      if (kind >= PCP_LT3 && kind <= PCP_MUL3) ++steps3; else ++steps2;
      rec_propagate_set(rec, dm);
    };
    bool failed = __builtin_amdgcn_readfirstlane(misc[S_FAIL]) != 0;
    while (!failed) {
      ++rounds;
      if (rounds > 1) {
        // the exact bounds of every variable the round before narrowed, from its words; an emptied set fails the node
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
      }
      const uint32_t before = narrow;
      for (uint32_t u = lane; u < U; u += 64) {
        if (!((live[u >> 5] >> (u & 31u)) & 1u)) continue;
        const uint32_t root = a.unit_root[u], n = a.unit_root[u + 1] - root;
        const FNode rn = a.nodes[root];
        bool entailed;
        if (n > 64u || rn.type == PCP_F_LEAF) {
          // a single propagator, or a flat Conjunction of leaves too wide for the masks: the members in order (conjunction.rs:97-104)
          const uint32_t m0 = rn.type == PCP_F_LEAF ? root : rn.first, m1 = rn.type == PCP_F_LEAF ? root + 1 : rn.first + rn.n_children;
          entailed = true;
          for (uint32_t k = m0; k < m1; ++k) {
            const Rec rec = a.m.recs[a.nodes[k].first];
            leaf_propagate(rec);
            entailed = entailed && rec_subsumed_set(rec, dm) == 1u;
          }
        } else {
          // bottom-up: is_subsumed() of every node of the tree (bit i = node root + i)
          unsigned long long t_true = 0, t_false = 0;
          for (uint32_t i = n; i-- > 0;) {
            const FNode nd = a.nodes[root + i];
            uint32_t s_;
            if (nd.type == PCP_F_LEAF) {
              s_ = rec_subsumed_set(a.m.recs[nd.first], dm);
            } else {
              const unsigned long long cm = (nd.n_children >= 64 ? ~0ull : ((1ull << nd.n_children) - 1ull)) << (nd.first - root);
              if (nd.type == PCP_F_AND) s_ = (t_false & cm) ? 0u : ((t_true & cm) == cm ? 1u : 2u);   // conjunction.rs:78-94
              else s_ = (t_true & cm) ? 1u : ((t_false & cm) == cm ? 0u : 2u);                          // disjunction.rs:78-94
            }
            if (s_ == 1u) t_true |= 1ull << i; else if (s_ == 0u) t_false |= 1ull << i;
          }
          entailed = (t_true & 1ull) != 0;
          if (!entailed) {
            // top-down: propagate()
            unsigned long long active = 1ull;
            for (uint32_t i = 0; i < n; ++i) {
              if (!((active >> i) & 1ull)) continue;
              const FNode nd = a.nodes[root + i];
              if (nd.type == PCP_F_LEAF) { leaf_propagate(a.m.recs[nd.first]); continue; }
              const unsigned long long cm = (nd.n_children >= 64 ? ~0ull : ((1ull << nd.n_children) - 1ull)) << (nd.first - root);
              if (nd.type == PCP_F_AND) { active |= cm; continue; }
              if (t_true & cm) continue;                                 // an entailed child: the Disjunction holds (disjunction.rs:103)
              const unsigned long long open = cm & ~t_false;             // the children that are not disentailed
              if (open == 0ull) dm.fail();                               // all disentailed (disjunction.rs:112-114)
              else if ((open & (open - 1ull)) == 0ull) active |= open;   // exactly one left: unit propagation (disjunction.rs:108-111)
            }
          }
        }
        if (entailed) atomicAnd(&live[u >> 5], ~(1u << (u & 31u)));      // unlink_prop (store.rs:200-207)
      }
      wave_sync();
      failed = __builtin_amdgcn_readfirstlane(misc[S_FAIL]) != 0;
      if (!__ballot(narrow != before)) break;
    }

    // ---- write back -----------------------------------------------------------------------------------------------------------------
    {
      uint64_t* dst = a.bits_out + row * sw;
      for (uint32_t i = lane; i < nwords; i += 64) dst[i] = bits[i];
    }
    for (uint32_t v = lane; v < V; v += 64) {
      const int2 b = bnd[v];
      a.lb_out[row + v] = b.x; a.ub_out[row + v] = b.y;
    }
    bool any_live = false;
    for (uint32_t w = lane; w < Wu; w += 64) any_live |= live[w] != 0;
    if (a.active_out)
      for (uint32_t w = lane; w < words64; w += 64) {
        const uint64_t lo = live[2 * w], hi = (2 * w + 1 < Wu) ? live[2 * w + 1] : 0u;
        a.active_out[(size_t)node * words64 + w] = lo | (hi << 32);
      }
    const bool unknown = __ballot(any_live) != 0;
    // Consistency::consistency (store.rs:250-256): False if a propagate failed, True if no subscription remains, else Unknown
    if (lane == 0) a.status[node] = failed ? (uint8_t)PCP_FALSE : (unknown ? (uint8_t)PCP_UNKNOWN : (uint8_t)PCP_TRUE);
    for (int o = 32; o > 0; o >>= 1) { steps2 += __shfl_down(steps2, o); steps3 += __shfl_down(steps3, o); narrow += __shfl_down(narrow, o); }
    acc_s2 += steps2; acc_s3 += steps3; acc_narrow += narrow; acc_waves += rounds ? rounds : 1; acc_nodes += 1; acc_failed += failed ? 1 : 0;
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

}  // namespace

size_t lds_bytes_setform(uint32_t n_vars, uint32_t set_words, uint32_t n_units, uint32_t waves) {
  const SetFormCarve c = setform_carve(n_vars, set_words, n_units);
  return c.total * waves <= 160 * 1024 ? c.total * waves : 0;
}

hipError_t launch_setformfix(const SetFormArgs& a, bool implicit, const LaunchPlan& p, hipStream_t stream) {
  const void* fn = implicit ? reinterpret_cast<const void*>(setformfix_kernel<true>) : reinterpret_cast<const void*>(setformfix_kernel<false>);
  if (p.lds_bytes > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes);
    if (e != hipSuccess) return e;
  }
  if (implicit) hipLaunchKernelGGL(setformfix_kernel<true>, dim3(p.grid), dim3(p.block), p.lds_bytes, stream, a);
  else hipLaunchKernelGGL(setformfix_kernel<false>, dim3(p.grid), dim3(p.block), p.lds_bytes, stream, a);
  return hipGetLastError();
}

}  // namespace pcp
