// pcp_small.hpp — what the two kernels over SMALL Interval<i32> stores share: the carve of a workgroup's LDS (the records' copy all its
// wavefronts read, then one slice per wavefront), the cooperative copy into the shared part, and one ROUND of the fixpoint — every
// all-different unit as a group, then every record of a live unit, with the `ent` bookkeeping and the step counts.  smallfix_kernel
// (pcp_small.hip: the fixpoint of a batch of nodes) and smalldfs_kernel (pcp_smalldfs.hip: SmallNode::propagate inside row_dfs, pcp_rowdfs.hpp — the search loop, one tree per wavefront) run it on
// LdsDom, the node's (-lb, ub) cells in LDS.  The records' twin of pcp_formula.hpp.  Device code only; everything lives in an unnamed
// namespace.
#pragma once
#include "pcp_device.hpp"
#include "pcp_neq.h"

namespace pcp {

namespace {

enum { S_FAIL = 0, S_OOB = 1, S_TAKEN = 4 /* .. 7 */, S_WORDS = 8 };
constexpr uint32_t kSmallAdUnits = 8;    // all-different units filtered as groups (more of them: the later ones run pair by pair)
constexpr uint32_t kSmallAdVars = 256;   // their variables, all together
constexpr uint32_t kSmallAdWords = 1 + 3 * kSmallAdUnits + kSmallAdVars;

// the workgroup's shared part of LDS: the records, their unit ids (u16), the all-different tables
__host__ __device__ inline size_t small_shared_off(uint32_t P, int part) {
  auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
  const size_t o_unit = up((size_t)P * sizeof(Rec)), o_ad = o_unit + up((size_t)P * 2), o_end = o_ad + up((size_t)kSmallAdWords * 4);
  return part == 0 ? o_unit : part == 1 ? o_ad : o_end;
}
__host__ __device__ inline size_t small_shared_bytes(uint32_t P) { return small_shared_off(P, 2); }

// one wavefront's slice: cells, a (dummy) changed mask, the live units, the entailed units, flags
__host__ __device__ inline size_t small_wave_bytes(uint32_t S, uint32_t U) {
  auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
  return up((size_t)S * 8) + up((size_t)((S + 31) / 32) * 4) + 2 * up((size_t)((U + 31) / 32) * 4) + up(S_WORDS * 4);
}

struct SmallShared {
  const Rec* recs;        // [P]
  const uint16_t* runit;  // [P] the unit of each record
  const uint32_t* adt;    // [n, (unit, count, first) * n]
  const uint32_t* adv;    // the all-different units' variables
  uint32_t n_ad;
};

struct SmallSlice {
  int2* dom;       // [S] (-lb, ub)
  uint32_t* chg;   // [ceil(S / 32)]
  uint32_t* live;  // [ceil(U / 32)]
  uint32_t* ent;   // [ceil(U / 32)]
  uint32_t* misc;  // [S_WORDS]
};

__device__ __forceinline__ SmallSlice small_slice(unsigned char* smem, uint32_t P, uint32_t S, uint32_t U, uint32_t wv) {
  auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
  const uint32_t Wu = (U + 31) >> 5, Wv = (S + 31) >> 5;
  unsigned char* const mine = smem + small_shared_bytes(P) + (size_t)wv * small_wave_bytes(S, U);
  SmallSlice s;
  s.dom = reinterpret_cast<int2*>(mine);
  s.chg = reinterpret_cast<uint32_t*>(mine + up((size_t)S * 8));
  s.live = s.chg + (up((size_t)Wv * 4) >> 2);
  s.ent = s.live + (up((size_t)Wu * 4) >> 2);
  s.misc = s.ent + (up((size_t)Wu * 4) >> 2);
  return s;
}

__device__ __forceinline__ void small_wave_sync() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier(); }

// The workgroup's copy of the records, then the all-different tables: [n, (unit, count, first) * n] then the variables, kSmallAdWords words in
// all (the host checks that they fit).  EVERY thread of the workgroup calls this; the caller takes the __syncthreads() that publishes it.
// (Everything a round reads comes from LDS: with the unit ids and the all-different tables in global memory a lane's round was a chain
// of dependent L2 round trips, one per record — 0.26 ms for config 4 where the filters themselves take a fifth of that)
__device__ __forceinline__ SmallShared small_copy_shared(unsigned char* smem, uint32_t P, const Rec* g_recs, const uint32_t* g_rec_unit, const uint32_t* g_ad_tab,
                                                         const uint32_t* g_ad_vars) {
  auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
  const uint32_t tid = threadIdx.x;
  Rec* const recs = reinterpret_cast<Rec*>(smem);
  uint16_t* const runit = reinterpret_cast<uint16_t*>(smem + up((size_t)P * sizeof(Rec)));
  uint32_t* const adt = reinterpret_cast<uint32_t*>(smem + small_shared_off(P, 1));
  for (uint32_t r = tid; r < P; r += blockDim.x) { recs[r] = g_recs[r]; runit[r] = (uint16_t)(g_rec_unit ? g_rec_unit[r] : r); }
  const uint32_t n_ad = g_ad_tab ? min(g_ad_tab[0], kSmallAdUnits) : 0u;
  if (n_ad) {
    const uint32_t n_vars_ad = g_ad_tab[3 * n_ad] + g_ad_tab[3 * n_ad - 1];  // first + count of the last unit
    for (uint32_t i = tid; i < 1 + 3 * n_ad; i += blockDim.x) adt[i] = g_ad_tab[i];
    for (uint32_t i = tid; i < n_vars_ad; i += blockDim.x) adt[1 + 3 * kSmallAdUnits + i] = g_ad_vars[i];
  }
  return SmallShared{recs, runit, adt, adt + 1 + 3 * kSmallAdUnits, n_ad};
}

// ONE ROUND of a node's fixpoint, by its wavefront: a live unit counts as entailed (`ent`) until one of its members says otherwise;
// `node_units(...)` (the node's own propagators: smallfix_kernel; the search loop: row_dfs's exclusion sweep under Enumerate, else nothing) runs first; then the all-different units, then
// every record of a live unit, lane-strided.  A round that narrows nothing has evaluated every live record on the final domains, so its
// `ent` IS the units' entailment.  The caller takes the wavefront barrier after the round, reads misc[S_FAIL] and compares ctr.narrow.
template <class NodeUnits>
__device__ __forceinline__ void small_round(const SmallShared& sh, uint32_t P, uint32_t Wu, const SmallSlice& sl, const LdsDom& dm, uint32_t lane, uint32_t& s2,
                                            uint32_t& s3, NodeUnits&& node_units) {
  const Rec* const recs = sh.recs;
  const uint16_t* const runit = sh.runit;
  const uint32_t* const adt = sh.adt;
  const uint32_t* const adv = sh.adv;
  const uint32_t n_ad = sh.n_ad;
  int2* const dom = sl.dom;
  uint32_t* const live = sl.live;
  uint32_t* const ent = sl.ent;
  uint32_t* const misc = sl.misc;
  for (uint32_t w = lane; w < Wu; w += 64) ent[w] = live[w];  // a live unit counts as entailed until one of its members says otherwise
  small_wave_sync();
  node_units();
  unsigned long long grouped = 0;  // (wave-uniform) the all-different units filtered as a group this round: bit k = entry k of ad_tab
  for (uint32_t k = 0; k < n_ad; ++k) {
    const uint32_t au = adt[1 + 3 * k], cnt = adt[2 + 3 * k], v0 = adt[3 + 3 * k];
    if (!((live[au >> 5] >> (au & 31u)) & 1u)) continue;
    const bool on = lane < cnt;
    const uint32_t v = on ? adv[v0 + lane] : 0u;
    int2 d = make_int2(0, 0);
    if (on) { const int2 c_ = dom[v]; d = make_int2(-c_.x, c_.y); }
    int lo = on ? d.x : 0x7fffffff, hi = on ? d.y : (int)0x80000000;
    for (int o = 32; o > 0; o >>= 1) { lo = min(lo, __shfl_xor(lo, o)); hi = max(hi, __shfl_xor(hi, o)); }
    if ((long long)hi - (long long)lo >= 128) continue;  // (wave-uniform) too wide for the mask: this unit's pairs run below
    grouped |= 1ull << k;
    if (lane < 4) misc[S_TAKEN + lane] = 0;
    small_wave_sync();
    if (lane == 0) s2 += cnt * (cnt - 1u) / 2u;  // the unit's cnt (cnt - 1) / 2 pair filters, what the reference (and small_alldiff = 0) runs and counts for it in one round
    const bool single = on && d.x == d.y;
    if (single) {
      const uint32_t b = (uint32_t)(d.x - lo);
      if (atomicOr(&misc[S_TAKEN + (b >> 5)], 1u << (b & 31u)) & (1u << (b & 31u))) dm.set_fail();  // two variables, one value
    }
    small_wave_sync();
    if (on && !single) {
      // the 128 value bits as two 64-bit registers.  (Made opaque: left to itself the compiler turns "pick one of four loaded words"
      // into "pick one of four ADDRESSES, then load", through an array of pointers in scratch memory — 72 bytes per lane.)
      unsigned long long tlo = (unsigned long long)misc[S_TAKEN] | ((unsigned long long)misc[S_TAKEN + 1] << 32);
      unsigned long long thi = (unsigned long long)misc[S_TAKEN + 2] | ((unsigned long long)misc[S_TAKEN + 3] << 32);
      asm volatile("" : "+v"(tlo), "+v"(thi));
      auto taken = [&](int val) { const uint32_t b = (uint32_t)(val - lo); return (((b < 64 ? tlo : thi) >> (b & 63u)) & 1ull) != 0; };
      int nl = d.x, nu = d.y;
      while (nl <= nu && taken(nl)) ++nl;
      while (nu >= nl && taken(nu)) --nu;
      if (nl > d.x) dm.raise_lb(v, nl);
      if (nu < d.y && nu >= nl) dm.lower_ub(v, nu);
      if (nl > nu) dm.set_fail();
    }
    small_wave_sync();
    // the unit's is_subsumed(): True iff every pair is disjoint (conjunction.rs:78-94 over x_neq_y.rs:71-73).  More values claimed than
    // the hull has room for is an overlap somewhere (the usual case, one wave sum); otherwise every lane looks at every other interval.
    {
      int l2 = 0, u2 = -1;
      if (on) { const int2 c2 = dom[v]; l2 = -c2.x; u2 = c2.y; }
      uint32_t claimed = on && u2 >= l2 ? (uint32_t)(u2 - l2 + 1) : 0u;
      for (int o = 32; o > 0; o >>= 1) claimed += __shfl_xor(claimed, o);
      bool overlap = claimed > (uint32_t)(hi - lo + 1);
      if (!overlap) {
        bool ov = false;
        for (uint32_t j = 0; j < cnt; ++j) {
          const int lj = __builtin_amdgcn_readlane(l2, (int)j), uj = __builtin_amdgcn_readlane(u2, (int)j);
          ov |= on && j != lane && !(u2 < lj || uj < l2);
        }
        overlap = __ballot(ov) != 0;
      }
      if (overlap && lane == 0) atomicAnd(&ent[au >> 5], ~(1u << (au & 31u)));
    }
  }
  for (uint32_t r = lane; r < P; r += 64) {
    const uint32_t u = runit[r];
    if (!((live[u >> 5] >> (u & 31u)) & 1u)) continue;
    if (grouped) {  // a member of an all-different unit that was filtered as a group this round?
      bool skip = false;
      for (uint32_t k = 0; k < n_ad; ++k) skip |= ((grouped >> k) & 1ull) && adt[1 + 3 * k] == u;
      if (skip) continue;
    }
    const Rec rec = recs[r];
    if ((rec.xk >> 28) >= PCP_LT3) ++s3; else ++s2;
    if (!eval_record(rec, dm)) atomicAnd(&ent[u >> 5], ~(1u << (u & 31u)));   // propagate_one + is_subsumed (store.rs:166-175)
  }
}

}  // namespace

}  // namespace pcp
