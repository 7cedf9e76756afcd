// pcp_setform.hpp — what the two kernels over formula stores on IntervalSet<i32> domains share: the LDS slice of one node (setform_carve),
// is_subsumed() / propagate() of an elementary leaf on sets, and the step of one formula unit.  setformfix_kernel (pcp_setform.hip: the
// fixpoint of a batch of nodes) runs them on SetDomT<false>, setformdfs_kernel (pcp_setformdfs.hip: the search loop, one tree per
// wavefront) on SetDomT<true>, so that every narrowing is logged to the tree's undo trail.  Everything here is __forceinline__: an
// out-of-line leaf costs scratch.  Device code only.
#pragma once
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
  c.misc = o; o = up(o + 32 * 4);  // the S_* words SetDomT names (S_FAIL; S_TRAILOVF and S_TRAILLEN only with a trail)
  c.total = o;
  return c;
}

__device__ __forceinline__ uint32_t kleene_and(uint32_t a, uint32_t b) { return (a == 0u || b == 0u) ? 0u : ((a == 1u && b == 1u) ? 1u : 2u); }
__device__ __forceinline__ uint32_t kleene_not(uint32_t a) { return a == 2u ? 2u : 1u - a; }

// is_subsumed() of one elementary propagator as SKleene (0 False, 1 True, 2 Unknown), on IntervalSet<i32> domains:
//   XEqY x_eq_y.rs:73-94 (False iff the SETS are disjoint) | XNeqY x_neq_y.rs:71-73 (not XEqY) | XLessY x_less_y.rs:73-95 |
//   XLessYPlusZ x_less_y_plus_z.rs:82-97 | XGreaterYPlusZ x_greater_y_plus_z.rs:82-98 | XEqYPlusZ x_eq_y_plus_z.rs:60-67 (Kleene and of
//   its halves) | Boolean boolean.rs:111-127 | BooleanNeg boolean_neg.rs:71-79.  A Constant operand is a singleton without words.
template <class DM>
__device__ __forceinline__ uint32_t rec_subsumed_set(const Rec& rec, const DM& dm) {
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
template <class DM>
__device__ __forceinline__ void rec_propagate_set(const Rec& rec, const DM& dm) {
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

// One step of formula unit u on the node `dm`: propagate() of the unit's tree (nodes[unit_root[u] .. unit_root[u + 1]), breadth first) and
// whether the unit is entailed, in which case the caller unlinks it (unlink_prop, store.rs:200-207).  A tree of up to 64 nodes is walked by
// two loops with 64-bit masks — bottom-up is_subsumed() of every node, then top-down propagate() of the active ones; a single propagator, or
// a flat Conjunction of leaves too wide for the masks, runs its members in order (conjunction.rs:97-104).  steps2 / steps3 count the leaf
// propagate() calls by arity.
template <class DM>
__device__ __forceinline__ bool setform_unit_step(const FNode* __restrict__ nodes, const uint32_t* __restrict__ unit_root, const Rec* __restrict__ recs,
                                                  uint32_t u, const DM& dm, uint32_t& steps2, uint32_t& steps3) {
  auto leaf_propagate = [&](const Rec& rec) {
    const uint32_t kind = rec.xk >> 28;
    if (kind >= PCP_LT3 && kind <= PCP_MUL3) ++steps3; else ++steps2;
    rec_propagate_set(rec, dm);
  };
  const uint32_t root = unit_root[u], n = unit_root[u + 1] - root;
  const FNode rn = nodes[root];
  bool entailed;
  if (n > 64u || rn.type == PCP_F_LEAF) {
    const uint32_t m0 = rn.type == PCP_F_LEAF ? root : rn.first, m1 = rn.type == PCP_F_LEAF ? root + 1 : rn.first + rn.n_children;
    entailed = true;
    for (uint32_t k = m0; k < m1; ++k) {
      const Rec rec = recs[nodes[k].first];
      leaf_propagate(rec);
      entailed = entailed && rec_subsumed_set(rec, dm) == 1u;
    }
  } else {
    // bottom-up: is_subsumed() of every node of the tree (bit i = node root + i)
    unsigned long long t_true = 0, t_false = 0;
    for (uint32_t i = n; i-- > 0;) {
      const FNode nd = nodes[root + i];
      uint32_t s_;
      if (nd.type == PCP_F_LEAF) {
        s_ = rec_subsumed_set(recs[nd.first], dm);
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
        const FNode nd = nodes[root + i];
        if (nd.type == PCP_F_LEAF) { leaf_propagate(recs[nd.first]); continue; }
        const unsigned long long cm = (nd.n_children >= 64 ? ~0ull : ((1ull << nd.n_children) - 1ull)) << (nd.first - root);
        if (nd.type == PCP_F_AND) { active |= cm; continue; }
        if (t_true & cm) continue;                                 // an entailed child: the Disjunction holds (disjunction.rs:103)
        const unsigned long long open = cm & ~t_false;             // the children that are not disentailed
        if (open == 0ull) dm.fail();                               // all disentailed (disjunction.rs:112-114)
        else if ((open & (open - 1ull)) == 0ull) active |= open;   // exactly one left: unit propagation (disjunction.rs:108-111)
      }
    }
  }
  return entailed;
}

}  // namespace

}  // namespace pcp
