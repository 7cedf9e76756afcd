// pcp_formula.hpp — what the two kernels over formula stores on Interval<i32> domains share: the LDS slice of one node (form_carve),
// is_subsumed() / propagate() of an elementary leaf, and the step of one formula unit.  formfix_kernel (pcp_formula.hip: the fixpoint of a
// batch of nodes) and formdfs_kernel (pcp_formdfs.hip: FormulaNode::propagate inside row_dfs, pcp_rowdfs.hpp — the search loop, one tree per wavefront) run them on LdsDom, the node's (-lb, ub)
// cells in LDS.  The interval twin of pcp_setform.hpp.  Device code only; everything lives in an unnamed namespace.
#pragma once
#include "pcp_device.hpp"
#include "pcp_neq.h"

namespace pcp {

namespace {

enum { F_FAIL = 0, F_OOB = 1, F_CHANGED = 2, F_STEPS2 = 4, F_STEPS3 = 6, F_NARROW = 8, F_WAVES = 9, F_WORDS = 10 };

struct FormCarve {
  size_t dom, chg, live, misc, total;
};
__host__ __device__ inline FormCarve form_carve(uint32_t S, uint32_t U) {
  auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
  FormCarve c;
  size_t o = 0;
  c.dom = o; o = up(o + (size_t)S * 8);
  c.chg = o; o = up(o + (size_t)((S + 31) / 32) * 4);
  c.live = o; o = up(o + (size_t)((U + 31) / 32) * 4);
  c.misc = o; o = up(o + 16 * 4);
  c.total = o;
  return c;
}

// is_subsumed() of one elementary propagator as SKleene (0 False, 1 True, 2 Unknown), on Interval<i32> domains:
//   XEqY x_eq_y.rs:73-94 | XNeqY x_neq_y.rs:71-73 (not XEqY) | XLessY x_less_y.rs:73-95 | XLessYPlusZ x_less_y_plus_z.rs:82-97 |
//   XGreaterYPlusZ x_greater_y_plus_z.rs:82-98 | XEqYPlusZ x_eq_y_plus_z.rs:60-67 (Kleene and of its halves, cmp/mod.rs:62-86) |
//   XEqYMulZ x_eq_y_mul_z.rs:73-91 | Boolean boolean.rs:111-127 | BooleanNeg boolean_neg.rs:71-79.
__device__ __forceinline__ uint32_t kleene_and(uint32_t a, uint32_t b) { return (a == 0u || b == 0u) ? 0u : ((a == 1u && b == 1u) ? 1u : 2u); }
__device__ __forceinline__ uint32_t kleene_not(uint32_t a) { return a == 2u ? 2u : 1u - a; }

__device__ uint32_t rec_subsumed(const Rec& rec, const LdsDom& dm) {
  const uint32_t kind = rec.xk >> 28, x = rec.xk & kSlotMask;
  const long long d = rec.d;
  const int2 X = dm.load(x);
  if (kind == PCP_BOOL || kind == PCP_NBOOL) {  // the view is x + d; Boolean: singleton ? (value == 1) : Unknown
    uint32_t b = 2u;
    if (X.x == X.y) b = ((long long)X.x + d == 1) ? 1u : 0u;
    return kind == PCP_BOOL ? b : kleene_not(b);
  }
  const int2 Y = dm.load(rec.y);
  if (kind <= PCP_LT) {
    const long long Yl = (long long)Y.x + d, Yu = (long long)Y.y + d;
    if (kind == PCP_LT) return X.x >= Yu ? 0u : (X.y < Yl ? 1u : 2u);
    const uint32_t eq = (X.x == Yu && X.y == Yl) ? 1u : ((X.x > Yu || Yl > X.y) ? 0u : 2u);
    return kind == PCP_EQ ? eq : kleene_not(eq);
  }
  const int2 Z = dm.load(rec.z);
  auto lt3 = [&](long long dd) -> uint32_t {  // x < y + z + dd
    return (long long)X.x >= (long long)Y.y + Z.y + dd ? 0u : ((long long)X.y < (long long)Y.x + Z.x + dd ? 1u : 2u);
  };
  auto gt3 = [&](long long dd) -> uint32_t {  // x > y + z + dd
    return (long long)X.y <= (long long)Y.x + Z.x + dd ? 0u : ((long long)X.x > (long long)Y.y + Z.y + dd ? 1u : 2u);
  };
  if (kind == PCP_LT3) return lt3(d);
  if (kind == PCP_GT3) return gt3(d);
  if (kind == PCP_EQ3) return kleene_and(gt3(d - 1), lt3(d + 1));
  // XEqYMulZ: (x + dx) = (y + dy) * (z + dz)
  const int32_t* mo = dm.mul_offsets() + 3 * (size_t)rec.d;
  const long long yl = Y.x + (long long)mo[1], yu = Y.y + (long long)mo[1], zl = Z.x + (long long)mo[2], zu = Z.y + (long long)mo[2];
  const long long p0 = yl * zl, p1 = yl * zu, p2 = yu * zl, p3 = yu * zu;
  const long long pl = min(min(p0, p1), min(p2, p3)), pu = max(max(p0, p1), max(p2, p3));
  const long long xl = X.x + (long long)mo[0], xu = X.y + (long long)mo[0];
  if (pl > xu || xl > pu) return 0u;
  return (pl == pu && xl == xu) ? 1u : 2u;
}

// propagate() of one elementary leaf.  A failure raises the node's fail flag (every caller ends the node on it).
__device__ void rec_propagate(const Rec& rec, const LdsDom& dm) {
  const uint32_t kind = rec.xk >> 28;
  if (kind == PCP_BOOL || kind == PCP_NBOOL) {
    // Boolean::propagate = update(var, {1}) (boolean.rs:134-137); BooleanNeg: {0} (boolean_neg.rs:86-89).  A domain without that
    // value is a non-monotonic update — the reference panics (variable/store.rs:153-156); here the node fails (pcp_hip.h).
    const uint32_t x = rec.xk & kSlotMask;
    const int want = (kind == PCP_BOOL ? 1 : 0) - rec.d;
    const int2 X = dm.load(x);
    if (want < X.x || want > X.y) { dm.set_fail(); return; }
    if (want > X.x) dm.raise_lb(x, want);
    if (want < X.y) dm.lower_ub(x, want);
    return;
  }
  (void)eval_record(rec, dm);
}

// One step of formula unit u on the node `dm`: propagate() of the unit's tree and whether the unit is entailed, in which case the caller
// unlinks it (unlink_prop, store.rs:200-207).  A unit's tree is laid out breadth-first — every child behind its parent, the children of a
// node consecutive (pcp_model_push_formula checks it) — so both walks are LOOPS over the unit's nodes[unit_root[u] .. unit_root[u + 1]):
//   bottom-up  (last node to first): is_subsumed() of every node from its children's, kept as two bit masks (true / false) in registers;
//   top-down   (first to last): propagate() — an `active` bit mask starts at the root; an active Conjunction activates all its children
//              (conjunction.rs:97-104), an active Disjunction none if a child is entailed, its single not-disentailed child if there is exactly
//              one, and fails the node if there is none (disjunction.rs:97-117); an active leaf runs its filter.
// The Disjunction decides on the statuses the bottom-up walk found a moment earlier, where the reference asks its children while it runs: a
// decision on an older domain is the conservative one (is_subsumed() only ever moves from Unknown to True or False as domains shrink), the
// round after repeats it on the newer one, and the last round — the one that narrows nothing — sees final domains throughout.
// A unit whose root is entailed is not propagated: its propagate() is a no-op (disjunction.rs:103).
// Units of more than 64 nodes are flat Conjunctions of leaves (Distinct next to formulas): a loop over the members, like a single propagator.
// steps2 / steps3 count the leaf propagate() calls by arity.
__device__ __forceinline__ bool form_unit_step(const FNode* __restrict__ nodes, const uint32_t* __restrict__ unit_root, const Rec* __restrict__ recs,
                                               uint32_t u, const LdsDom& dm, uint32_t& steps2, uint32_t& steps3) {
  auto leaf_propagate = [&](const Rec& rec) {
    const uint32_t kind = rec.xk >> 28;
    if (kind >= PCP_LT3 && kind <= PCP_MUL3) ++steps3; else ++steps2;
    rec_propagate(rec, dm);
  };
  const uint32_t root = unit_root[u], n = unit_root[u + 1] - root;
  const FNode rn = nodes[root];
  bool entailed;
  if (n > 64u || rn.type == PCP_F_LEAF) {
    // a single propagator, or a flat Conjunction of leaves too wide for the masks: the members in order (conjunction.rs:97-104)
    const uint32_t m0 = rn.type == PCP_F_LEAF ? root : rn.first, m1 = rn.type == PCP_F_LEAF ? root + 1 : rn.first + rn.n_children;
    entailed = true;
    for (uint32_t k = m0; k < m1; ++k) {
      const Rec rec = recs[nodes[k].first];
      leaf_propagate(rec);
      entailed = entailed && rec_subsumed(rec, dm) == 1u;
    }
  } else {
    // bottom-up: is_subsumed() of every node of the tree (bit i = node root + i)
    unsigned long long t_true = 0, t_false = 0;
    for (uint32_t i = n; i-- > 0;) {
      const FNode nd = nodes[root + i];
      uint32_t s_;
      if (nd.type == PCP_F_LEAF) {
        s_ = rec_subsumed(recs[nd.first], dm);
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
        if (open == 0ull) dm.set_fail();                           // all disentailed (disjunction.rs:112-114)
        else if ((open & (open - 1ull)) == 0ull) active |= open;   // exactly one left: unit propagation (disjunction.rs:108-111)
      }
    }
  }
  return entailed;
}

}  // namespace

}  // namespace pcp
