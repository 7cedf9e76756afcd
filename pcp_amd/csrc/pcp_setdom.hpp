// pcp_setdom.hpp — IntervalSet<i32> domains as bitsets in LDS: the domain object the set-mode kernels narrow (SetDomT), the elementary
// filters on it (eval_set), the bounds of a set from its words (scan_bounds) and the member of a set nearest to a value (Enumerate's
// value rule).  Shared by the kernels of pcp_set.hip (one workgroup per node, plain stores) and of pcp_setform.hip / pcp_setformdfs.hip
// (one wavefront per node or per tree, stores with formula propagators).  Device code only.
#pragma once
#include "pcp_internal.h"

namespace pcp {

namespace {

// words of a node's `misc` area in LDS.  SetDomT itself touches S_FAIL and S_TRAILOVF only; the rest belongs to the kernels of pcp_set.hip.
enum { S_FAIL = 0, S_TOTAL = 1, S_ITEMS = 2, S_TOTAL2 = 3, S_ITEMS2 = 4, S_WAVES = 5, S_OPEN = 6, S_NARROW = 7, S_STEPS2 = 8, S_STEPS3 = 10, S_EVAL = 12, S_LIVE = 14, S_NSING = 15,
       S_TRAILOVF = 16, S_TRAILLEN = 17, S_CTL = 18 /* .. 23: the DFS loop's broadcast words */ };

// One node's domains in LDS.  TRAIL = true (the device-side DFS, setdfs_kernel): every narrowing also appends (word, removed bits)
// to the tree's undo trail, which is what the reference's VStoreTrail keeps (variable/memory/trail_memory.rs:100-104): a
// backtrack ORs the removed bits back instead of reloading a node.
template <bool TRAIL>
struct SetDomT {
  unsigned long long* bits;  // [V][sw]
  int2* bnd;                 // [V] (lb, ub)
  const int32_t* cval;       // constants, slots >= V
  uint32_t V, sw;
  int32_t base;
  uint32_t* chg;             // changed mask to mark
  uint32_t* misc;
  uint32_t* narrow;          // per-thread counter
  uint4* trail = nullptr;    // TRAIL: the tree's trail in HBM, its length (an LDS word) and its capacity
  uint32_t* trail_len = nullptr;
  uint32_t trail_cap = 0;

  __device__ __forceinline__ void log(uint32_t var, uint32_t widx, unsigned long long removed) const {
    if constexpr (TRAIL) {
      if (!removed) return;
      const uint32_t pos = atomicAdd(trail_len, 1u);
      if (pos < trail_cap) trail[pos] = make_uint4(widx, var, (uint32_t)removed, (uint32_t)(removed >> 32));
      else atomicOr(&misc[S_TRAILOVF], 1u);
    }
  }

  __device__ __forceinline__ bool is_const(uint32_t s) const { return s >= V; }
  __device__ __forceinline__ int2 bounds(uint32_t s) const {
    if (s >= V) { const int c = cval[s - V]; return make_int2(c, c); }
    return bnd[s];
  }
  __device__ __forceinline__ void fail() const { atomicOr(&misc[S_FAIL], 1u); }
  __device__ __forceinline__ void mark(uint32_t s) const { atomicOr(&chg[s >> 5], 1u << (s & 31)); ++*narrow; }
  __device__ __forceinline__ bool test(uint32_t s, int v) const {  // v in the set of slot s?
    if (s >= V) return cval[s - V] == v;
    const long long b = (long long)v - base;
    if (b < 0 || b >= (long long)sw * 64) return false;
    return (bits[(size_t)s * sw + (b >> 6)] >> (b & 63)) & 1ull;
  }
  // IntervalSet::difference(&v): remove ONE value (x_neq_y.rs:86-89).  Removing the value of a Constant empties it:
  // Constant::update returns false (term/constant.rs:49-52).
  __device__ __forceinline__ void remove(uint32_t s, int v) const {
    if (s >= V) { if (cval[s - V] == v) fail(); return; }
    const long long b = (long long)v - base;
    if (b < 0 || b >= (long long)sw * 64) return;
    const unsigned long long m = 1ull << (b & 63);
    unsigned long long* w = &bits[(size_t)s * sw + (b >> 6)];
    if (!(*w & m)) return;
    if (atomicAnd(w, ~m) & m) { log(s, s * sw + (uint32_t)(b >> 6), m); mark(s); }
  }
  // keep only the values <= t  (shrink_right) / >= t (shrink_left), within the cached bounds [lo, hi] of slot s
  __device__ __forceinline__ void keep_le(uint32_t s, long long t, const int2 cur) const {
    if (t >= cur.y) return;
    if (s >= V) { fail(); return; }  // a constant above t
    clear_range(s, t + 1, cur.y);
  }
  __device__ __forceinline__ void keep_ge(uint32_t s, long long t, const int2 cur) const {
    if (t <= cur.x) return;
    if (s >= V) { fail(); return; }
    clear_range(s, cur.x, t - 1);
  }
  __device__ __forceinline__ void clear_range(uint32_t s, long long lo, long long hi) const {  // values lo..hi inclusive
    long long b0 = lo - base, b1 = hi - base;
    if (b0 < 0) b0 = 0;
    if (b1 >= (long long)sw * 64) b1 = (long long)sw * 64 - 1;
    if (b0 > b1) return;
    bool changed = false;
    for (long long k = b0 >> 6; k <= (b1 >> 6); ++k) {
      unsigned long long m = ~0ull;
      if (k == (b0 >> 6)) m &= ~0ull << (b0 & 63);
      if (k == (b1 >> 6)) m &= ~0ull >> (63 - (b1 & 63));
      unsigned long long* w = &bits[(size_t)s * sw + k];
      if (*w & m) {
        const unsigned long long gone = atomicAnd(w, ~m) & m;
        log(s, s * sw + (uint32_t)k, gone);
        changed |= gone != 0;
      }
    }
    if (changed) mark(s);
  }
  // 64 bits of slot s starting at bit position pos (positions outside the universe read as 0)
  __device__ __forceinline__ unsigned long long window(uint32_t s, long long pos) const {
    const long long nb = (long long)sw * 64;
    if (pos <= -64 || pos >= nb) return 0ull;
    const long long k = pos >> 6;  // floor
    const int sh = (int)(pos & 63);
    const unsigned long long lo = (k >= 0 && k < (long long)sw) ? bits[(size_t)s * sw + k] : 0ull;
    if (sh == 0) return lo;
    const unsigned long long hi = (k + 1 >= 0 && k + 1 < (long long)sw) ? bits[(size_t)s * sw + k + 1] : 0ull;
    return (lo >> sh) | (hi << (64 - sh));
  }
  // x := x ∩ (y + d) on the words of x
  __device__ __forceinline__ void intersect_shifted(uint32_t x, uint32_t y, long long d) const {
    if (x >= V) return;
    bool changed = false;
    for (uint32_t k = 0; k < sw; ++k) {
      unsigned long long* w = &bits[(size_t)x * sw + k];
      const unsigned long long cur = *w;
      if (!cur) continue;
      unsigned long long other;
      if (y >= V) {
        const long long b = (long long)cval[y - V] + d - base - (long long)k * 64;
        other = (b >= 0 && b < 64) ? (1ull << b) : 0ull;
      } else {
        other = window(y, (long long)k * 64 - d);  // value v of x  <->  value v - d of y
      }
      if (cur & ~other) {
        const unsigned long long gone = atomicAnd(w, other) & ~other;
        log(x, x * sw + k, gone);
        changed |= gone != 0;
      }
    }
    if (changed) mark(x);
  }
  // is x ∩ (y + d) empty?
  __device__ __forceinline__ bool disjoint_shifted(uint32_t x, uint32_t y, long long d) const {
    for (uint32_t k = 0; k < sw; ++k) {
      const unsigned long long cur = bits[(size_t)x * sw + k];
      if (cur && (cur & window(y, (long long)k * 64 - d))) return false;
    }
    return true;
  }
};
using SetDom = SetDomT<false>;

// One filter step on sets: propagate() + is_subsumed().  `want_entailed` = false skips the (possibly expensive) subsumption
// test — implicit-active nodes need it only in the final scan.  Returns whether the propagator is entailed.
template <class DM>
__device__ __forceinline__ bool eval_set(const Rec& rec, const DM& dm, const bool want_entailed) {
  const uint32_t kind = rec.xk >> 28, x = rec.xk & kSlotMask, y = rec.y;
  const long long d = rec.d;
  const int2 X = dm.bounds(x), Y = dm.bounds(y);
  if (X.x > X.y || Y.x > Y.y) return false;  // an emptied set: the node has failed (found by the next bounds step)
  if (kind == PCP_NEQ) {
    // XNeqY::propagate (x_neq_y.rs:82-93): a singleton side is removed from the other SET, wherever the value sits
    if (X.x == X.y) dm.remove(y, (int)(X.x - d));
    else if (Y.x == Y.y) dm.remove(x, (int)(Y.x + d));
    if (!want_entailed) return false;
    // !XEqY::is_subsumed (x_neq_y.rs:71-73, x_eq_y.rs:87-93): True iff the sets are disjoint
    if (X.x > Y.y + d || Y.x + d > X.y) return true;
    if (X.x == X.y) return !dm.test(y, (int)(X.x - d));
    if (Y.x == Y.y) return !dm.test(x, (int)(Y.x + d));
    if (dm.is_const(x) || dm.is_const(y)) return false;
    return dm.disjoint_shifted(x, y, d);
  }
  if (kind == PCP_EQ) {
    // XEqY::propagate (x_eq_y.rs:102-107): both become the intersection of the sets
    dm.intersect_shifted(x, y, d);
    dm.intersect_shifted(y, x, -d);
    if (dm.is_const(x) && dm.is_const(y) && X.x != Y.x + d) dm.fail();
    return want_entailed && X.x == X.y && Y.x == Y.y && X.x == Y.x + d;  // x_eq_y.rs:87-88
  }
  if (kind == PCP_LT) {
    // XLessY::propagate (x_less_y.rs:104-109): x.strict_shrink_right(y.upper()), y.strict_shrink_left(x.lower())
    dm.keep_le(x, (long long)Y.y + d - 1, X);
    dm.keep_ge(y, (long long)X.x - d + 1, Y);
    return (long long)X.y < (long long)Y.x + d;  // x_less_y.rs:90-91 (on the bounds read; re-evaluated while anything changes)
  }
  const uint32_t z = rec.z;
  const int2 Z = dm.bounds(z);
  if (Z.x > Z.y) return false;
  auto lt3 = [&](long long dd) {  // x < y + z + dd   (x_less_y_plus_z.rs:105-119)
    dm.keep_le(x, (long long)Y.y + Z.y + dd - 1, X);
    dm.keep_ge(y, (long long)X.x - Z.y - dd + 1, Y);
    dm.keep_ge(z, (long long)X.x - Y.y - dd + 1, Z);
  };
  auto gt3 = [&](long long dd) {  // x > y + z + dd   (x_greater_y_plus_z.rs:106-118)
    dm.keep_ge(x, (long long)Y.x + Z.x + dd + 1, X);
    dm.keep_le(y, (long long)X.y - Z.x - dd - 1, Y);
    dm.keep_le(z, (long long)X.y - Y.x - dd - 1, Z);
  };
  if (kind == PCP_LT3) { lt3(d); return (long long)X.y < (long long)Y.x + Z.x + d; }
  if (kind == PCP_GT3) { gt3(d); return (long long)X.x > (long long)Y.y + Z.y + d; }
  if (kind == PCP_EQ3) {  // geq && leq (x_eq_y_plus_z.rs:85-87; cmp/mod.rs:62-86)
    gt3(d - 1);
    lt3(d + 1);
    return (long long)X.x > (long long)Y.y + Z.y + d - 1 && (long long)X.y < (long long)Y.x + Z.x + d + 1;
  }
  dm.fail();  // XEqYMulZ on sets is rejected on the host (pcp_model_push_props)
  return false;
}

__device__ __forceinline__ int2 scan_bounds(const unsigned long long* w, uint32_t sw, int32_t base) {
  int lo = 1, hi = 0;
  for (uint32_t k = 0; k < sw; ++k)
    if (w[k]) { lo = base + (int)k * 64 + (int)__builtin_ctzll(w[k]); break; }
  for (uint32_t k = sw; k-- > 0;)
    if (w[k]) { hi = base + (int)k * 64 + 63 - (int)__builtin_clzll(w[k]); break; }
  return make_int2(lo, hi);
}

// The member of one variable's set (words w[0 .. sw), value = base + bit index) nearest to m, m - d before m + d, as a key for a minimum:
// 2 d for the nearest member <= m, 2 d + 1 for the nearest >= m (m itself: 0).  A word is reduced at once — the highest member <= m and the
// lowest member >= m of the masked word —, never value by value; the caller takes the minimum over the words.  ~0: no member in this word.
__device__ __forceinline__ unsigned long long nearest_member_key(unsigned long long w, long long word_lo, long long m) {
  const long long t = m - word_lo;  // m's bit in this word, if 0 <= t < 64
  const unsigned long long le = t < 0 ? 0ull : (t >= 63 ? ~0ull : ((2ull << t) - 1ull));  // the values <= m
  const unsigned long long ge = t <= 0 ? ~0ull : (t >= 64 ? 0ull : (~0ull << t));         // the values >= m
  unsigned long long key = ~0ull;
  const unsigned long long below = w & le, above = w & ge;
  if (below) key = 2ull * (unsigned long long)(m - (word_lo + 63 - __clzll((long long)below)));
  if (above) key = min(key, 2ull * (unsigned long long)(word_lo + (__ffsll((long long)above) - 1) - m) + 1ull);
  return key;
}
__device__ __forceinline__ long long nearest_member_value(unsigned long long key, long long m) {
  const long long d = (long long)(key >> 1);
  return (key & 1ull) ? m + d : m - d;
}

}  // namespace

}  // namespace pcp
