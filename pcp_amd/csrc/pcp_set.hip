// pcp_set.hip — the propagation fixpoint over IntervalSet<i32> domains (set mode), gfx950.
//
// The reference's default space is FDSpace = Space<VStoreSet, ...> with VStoreSet = VStoreTrail<IntervalSet<i32>>
// (variable/mod.rs:38, search/mod.rs:41-43; example/src/nqueens.rs:34 allocates IntervalSet::new(1, n)): domains are SETS, so
// XNeqY removes interior values (x_neq_y.rs:82-93 with IntervalSet::difference), variable::Store::update raises `Inner` events
// (events/mod.rs:57-64) and XEqY intersects sets (x_eq_y.rs:102-107).  Same engine semantics as the interval kernels
// (Store::consistency, propagation/store.rs:125-258): every live propagator once, then wake-up rounds until nothing changes.
//
// MI355X design: ONE workgroup (1024 threads, one CU) owns a node.  Its domains live in LDS for the whole fixpoint:
//   bits[V][set_words] u64   value v of variable x <-> bit (v - base) of bits[x]        (N-queens-1000: 1000 x 16 words = 125 KB)
//   bnd[V] (lb, ub)          the sets' bounds, exact at the start of every round
// A filter narrows a set with ds_and_b64 on the words it touches and marks the variable changed; it never writes the bounds.
// The first step of the next round re-derives the exact bounds of every changed variable from its words (ffs / clz) — between
// two such steps a filter may read bounds that are wider than the set, i.e. a superset of the current domain, which is the same
// benign race as in the interval kernels (monotone, contracting filters: the greatest fixpoint is unique).
// Wake-up rule: any change of a variable wakes all its propagators.  The reference wakes Bound-subscribers (XLessY and the
// ternary kinds) only on Bound/Assignment events, not on Inner ones (indexed_deps.rs:99-113) — but those filters read and
// write bounds only, so running them after an interior removal is a no-op: same fixpoint, a few more steps.
// Entailment (`active`, status True): XNeqY is entailed iff the two SETS are disjoint (x_eq_y.rs:87-93 through
// IntervalSet::is_disjoint), decided on the words (shifted intersection).
#include <algorithm>

#include "pcp_internal.h"
#include "pcp_setdom.hpp"  // SetDomT, eval_set, scan_bounds and the S_* words of `misc`
#include "pcp_setdfs.hpp"  // trail_dfs: the search loop of setdfs_kernel
#ifndef PCP_ABLATE
#define PCP_ABLATE 0  // profiling builds (tools/build_variant.py): bit 2048 = phase timers of setfix_kernel in the counters
#endif

namespace pcp {

namespace {

constexpr uint32_t kSetThreads = 1024;

struct SetCarve {
  size_t bits, bnd, chg_a, chg_b, list_id, list_off, list_deg, misc, total;
};
__host__ __device__ inline SetCarve set_carve(uint32_t V, uint32_t S, uint32_t sw, uint32_t cap) {
  auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
  const size_t Wv = (S + 31) / 32;
  SetCarve c;
  size_t o = 0;
  c.bits = o; o = up(o + (size_t)V * sw * 8);
  c.bnd = o; o = up(o + (size_t)V * 8);
  c.chg_a = o; o = up(o + Wv * 4);
  c.chg_b = o; o = up(o + Wv * 4);
  c.list_id = o; o = up(o + (size_t)cap * 4);
  c.list_off = o; o = up(o + (size_t)cap * 4);
  c.list_deg = o; o = up(o + (size_t)cap * 4);
  c.misc = o; o = up(o + 32 * 4);
  c.total = o;
  return c;
}

}  // namespace

size_t lds_bytes_set(uint32_t n_vars, uint32_t n_slots, uint32_t set_words, uint32_t list_cap) {
  const SetCarve c = set_carve(n_vars, n_slots, set_words, list_cap);
  return c.total <= 160 * 1024 ? c.total : 0;
}

struct SetArgs {
  ModelDev m;
  uint32_t n_nodes, set_words, list_cap;
  int32_t base;
  const uint64_t* bits_in;
  uint64_t* bits_out;
  int32_t* lb_out;
  int32_t* ub_out;
  const uint64_t* live_in;  // record-level rows or null
  uint64_t* live;           // null = implicit
  uint8_t* status;
  pcp_stats* stats;
};

template <bool IMPLICIT>
__global__ void __launch_bounds__(kSetThreads) setfix_kernel(const SetArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t tid = threadIdx.x, nth = blockDim.x, lane = tid & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6), nwv = nth >> 6;
  const uint32_t V = a.m.n_vars, S = a.m.n_slots, sw = a.set_words, C = a.list_cap, P = a.m.n_recs, words = (P + 63) >> 6;
  const uint32_t Wv = (S + 31) >> 5;
  const SetCarve cv = set_carve(V, S, sw, C);
  unsigned long long* bits = reinterpret_cast<unsigned long long*>(smem + cv.bits);
  int2* bnd = reinterpret_cast<int2*>(smem + cv.bnd);
  uint32_t* cur = reinterpret_cast<uint32_t*>(smem + cv.chg_a);
  uint32_t* nxt = reinterpret_cast<uint32_t*>(smem + cv.chg_b);
  uint32_t* list_id = reinterpret_cast<uint32_t*>(smem + cv.list_id);
  uint32_t* list_off = reinterpret_cast<uint32_t*>(smem + cv.list_off);
  uint32_t* list_deg = reinterpret_cast<uint32_t*>(smem + cv.list_deg);
  uint32_t* misc = reinterpret_cast<uint32_t*>(smem + cv.misc);
  const uint32_t node = blockIdx.x;
  pcp_stats* const st_slot = a.stats + (PCP_ABLATE ? 0u : (blockIdx.x & (kStatSlots - 1)));  // striped counters (pcp_internal.h)
  const uint64_t tail_mask = (P & 63) ? ((1ull << (P & 63)) - 1) : ~0ull;

  unsigned long long tph[6] = {0, 0, 0, 0, 0, 0};  // profiling build: phase boundaries (100 MHz ticks)
  if (PCP_ABLATE & 2048) tph[0] = wall_clock64();
  // ---- phase 0: stage the sets, derive their bounds ---------------------------------------------------------------------
  if (tid < 32) misc[tid] = 0;
  for (uint32_t i = tid; i < Wv; i += nth) { cur[i] = 0; nxt[i] = 0; }
  {
    const uint64_t* src = a.bits_in + (size_t)node * V * sw;
    const uint32_t nwords = V * sw;
    if (!(nwords & 1u) && !((size_t)src & 15)) {  // 16 bytes per lane: half the memory instructions of the node's 125 KB
      const uint4* s4 = reinterpret_cast<const uint4*>(src);
      uint4* d4 = reinterpret_cast<uint4*>(bits);
      for (uint32_t i = tid; i < nwords / 2; i += nth) d4[i] = s4[i];
    } else {
      for (uint32_t i = tid; i < nwords; i += nth) bits[i] = src[i];
    }
  }
  __syncthreads();
  for (uint32_t v = tid; v < V; v += nth) {
    const int2 b = scan_bounds(bits + (size_t)v * sw, sw, a.base);
    bnd[v] = b;
    if (b.x > b.y) atomicOr(&misc[S_FAIL], 1u);  // empty input domain
  }
  __syncthreads();

  uint32_t narrow = 0;
  uint64_t steps2 = 0, steps3 = 0;
  uint64_t* live_row = IMPLICIT ? nullptr : a.live + (size_t)node * words;
  if (PCP_ABLATE & 2048) tph[1] = wall_clock64();

  // ---- phase 1: every live propagator once (init_scheduler, store.rs:144-149) --------------------------------------------
  // Implicit nodes of an all-XNeqY model (N-queens): XNeqY::propagate is a no-op unless one operand is a singleton
  // (x_neq_y.rs:82-93), so of the whole sweep only the records of ASSIGNED variables can act: they are reached through the
  // variables' adjacency lists instead of streaming the table (N-queens-1000: a few thousand records instead of 1.5 million).
  // The other records count as reference-equivalent steps (the reference pops them) but are never looked at.
  uint64_t ev_only = 0;  // evaluated pairs that are not to be added to the credited steps again
  bool bulk_sweep = false;
  if constexpr (IMPLICIT) {
    bulk_sweep = a.m.uniform_kind == PCP_NEQ && S == V && !misc[S_FAIL];  // (a Constant operand has no adjacency: S == V excludes them)
    if (bulk_sweep) {
      for (uint32_t v = tid; v < V; v += nth) {
        const int2 b = bnd[v];
        if (b.x == b.y) {
          const uint32_t pos = atomicAdd(&misc[S_NSING], 1u);
          if (pos < C) list_id[pos] = v;
        }
      }
      __syncthreads();
      const uint32_t ns = misc[S_NSING];
      bulk_sweep = ns <= C;  // more assigned variables than the list holds: stream the table after all
      if (bulk_sweep) {
        const SetDom dm{bits, bnd, a.m.const_val, V, sw, a.base, cur, misc, &narrow};
        // four records per thread in flight; binary models rebuild the record from the adjacency payload (one coalesced
        // load instead of an index load and a gather that depends on it)
        constexpr int U = 4;
        for (uint32_t e = 0; e < ns; ++e) {
          const uint32_t v = list_id[e], o0 = a.m.adj_off[v], o1 = a.m.adj_off[v + 1];
          for (uint32_t i0 = o0 + tid; i0 < o1; i0 += nth * U) {
            Rec rc[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
              const uint32_t i = i0 + u * nth;
              const uint32_t at = i < o1 ? i : o0;
              if (a.m.adjp) {
                const uint2 q = a.m.adjp[at];
                const uint32_t other = q.x & kSlotMask, kind = (q.x >> 28) & 7u;
                const bool is_y = (q.x >> 31) != 0;
                rc[u].xk = (is_y ? other : v) | (kind << 28);
                rc[u].y = is_y ? v : other;
                rc[u].z = 0;
                rc[u].d = (int32_t)q.y;
              } else {
                rc[u] = a.m.recs[a.m.adj[at]];
              }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
              if (i0 + u * nth < o1) { (void)eval_set(rc[u], dm, false); ++ev_only; }
          }
        }
        if (tid == 0) { *reinterpret_cast<unsigned long long*>(&misc[S_STEPS2]) += (unsigned long long)P; misc[S_LIVE] = 1u; }
      }
    }
  }
  if (bulk_sweep) {
  } else if (!misc[S_FAIL]) {
    const uint64_t* in_row = (IMPLICIT || !a.live_in) ? nullptr : a.live_in + (size_t)node * words;
    const SetDom dm{bits, bnd, a.m.const_val, V, sw, a.base, cur, misc, &narrow};
    for (uint32_t w = wv; w < words; w += nwv) {
      const uint64_t raw = in_row ? in_row[w] : ~0ull;
      uint64_t word = raw;
      if (w == words - 1) word &= tail_mask;  // bits at or above n_recs name no record: they are dropped from the caller's row
      const uint32_t r = (w << 6) + lane;
      bool e = false;
      if ((word >> lane) & 1ull) {
        const Rec rec = a.m.recs[r];
        e = eval_set(rec, dm, !IMPLICIT);
        if ((rec.xk >> 28) > PCP_LT) ++steps3; else ++steps2;
      }
      if constexpr (!IMPLICIT) {
        const uint64_t nw = word & ~__ballot(e);
        if (lane == 0 && (in_row != live_row || nw != raw)) live_row[w] = nw;
      }
    }
  } else if constexpr (!IMPLICIT) {
    // failed while staging: the row that is exported must still be defined (the caller's row, or all units active)
    if (a.live_in != a.live || !a.live_in)
      for (uint32_t w = tid; w < words; w += nth) {
        uint64_t word = a.live_in ? a.live_in[(size_t)node * words + w] : ~0ull;
        if (w == words - 1) word &= tail_mask;
        live_row[w] = word;
      }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  if (PCP_ABLATE & 2048) tph[2] = wall_clock64();
  // ---- phase 2: wake-up rounds (react + schedule as waves, store.rs:191-198) --------------------------------------------
  const bool neq_only = IMPLICIT && a.m.uniform_kind == PCP_NEQ && S == V;
  for (uint32_t round = 0;; ++round) {
    const uint32_t m_total = (round & 1u) ? S_TOTAL2 : S_TOTAL, m_items = (round & 1u) ? S_ITEMS2 : S_ITEMS;
    // the exact bounds of every changed variable, from its words (an emptied set: the node has failed) — one thread per
    // variable: left to the compaction pass below (one thread per 32 variables) this rescan was most of a node's time
    for (uint32_t v = tid; v < V; v += nth) {
      if (!((cur[v >> 5] >> (v & 31)) & 1u)) continue;
      const int2 b = scan_bounds(bits + (size_t)v * sw, sw, a.base);
      bnd[v] = b;
      if (b.x > b.y) atomicOr(&misc[S_FAIL], 1u);
    }
    __syncthreads();
    {
      uint32_t degsum = 0;
      for (uint32_t w = tid; w < Wv; w += nth) {
        if (round) nxt[w] = 0;
        uint32_t bitsw = cur[w];
        if (!bitsw) continue;
        uint32_t dropped = 0;  // changed variables that wake nobody: taken out of `cur`, which the FIFO dedup below reads
        while (bitsw) {
          const uint32_t v = (w << 5) + __builtin_ctz(bitsw);
          bitsw &= bitsw - 1;
          if (v < V) {
            const int2 b = bnd[v];
            // all-XNeqY model, implicit node: a propagator acts only through a SINGLETON operand, so a variable that lost
            // values but is not assigned wakes nobody (the reference wakes all of them on its Inner event: no-op steps)
            if (neq_only && b.x != b.y) { dropped |= 1u << (v & 31); continue; }
          }
          const uint32_t pos = atomicAdd(&misc[m_total], 1u);
          if (pos < C) {
            const uint32_t o0 = (v < V) ? a.m.adj_off[v] : 0u, o1 = (v < V) ? a.m.adj_off[v + 1] : 0u;
            list_id[pos] = v; list_off[pos] = o0; list_deg[pos] = o1 - o0;
            degsum += o1 - o0;
          }
        }
        if (dropped) cur[w] &= ~dropped;
      }
      if (degsum) atomicAdd(&misc[m_items], degsum);
    }
    __syncthreads();
    const uint32_t total = misc[m_total];
    if (total == 0 || misc[S_FAIL]) break;
    if (tid == 0) { misc[S_WAVES] += 1; misc[(round & 1u) ? S_TOTAL : S_TOTAL2] = 0; misc[(round & 1u) ? S_ITEMS : S_ITEMS2] = 0; }
    const SetDom dm{bits, bnd, a.m.const_val, V, sw, a.base, nxt, misc, &narrow};
    auto run = [&](uint32_t v, uint32_t r) {
      // a record woken from variable v runs unless a lower-numbered changed variable of the same record runs it (FIFO dedup)
      if constexpr (!IMPLICIT) {
        if (!((live_row[r >> 6] >> (r & 63)) & 1ull)) return;  // unlinked (store.rs:200-207)
      }
      const Rec rec = a.m.recs[r];
      const uint32_t x = rec.xk & kSlotMask;
      const bool tern = (rec.xk >> 28) > PCP_LT;
      if (x < v && ((cur[x >> 5] >> (x & 31)) & 1u)) return;
      if (rec.y < v && ((cur[rec.y >> 5] >> (rec.y & 31)) & 1u)) return;
      if (tern && rec.z < v && ((cur[rec.z >> 5] >> (rec.z & 31)) & 1u)) return;
      if (tern) ++steps3; else ++steps2;
      const bool e = eval_set(rec, dm, !IMPLICIT);
      if constexpr (!IMPLICIT) {
        if (e) atomicAnd(reinterpret_cast<unsigned long long*>(&live_row[r >> 6]), ~(1ull << (r & 63)));
      }
    };
    if (total <= C) {
      // every (changed variable, incident record) pair: flat over the block, one list entry at a time per wavefront group
      for (uint32_t e = 0; e < total; ++e) {
        const uint32_t v = list_id[e], deg = list_deg[e], off = list_off[e];
        for (uint32_t i = tid; i < deg; i += nth) run(v, a.m.adj[off + i]);
      }
    } else {
      // more changed variables than the list holds: every record that touches a changed variable
      for (uint32_t r = tid; r < P; r += nth) {
        const Rec rec = a.m.recs[r];
        const uint32_t x = rec.xk & kSlotMask;
        const bool tern = (rec.xk >> 28) > PCP_LT;
        uint32_t vmin = 0xFFFFFFFFu;
        if ((cur[x >> 5] >> (x & 31)) & 1u) vmin = x;
        if (((cur[rec.y >> 5] >> (rec.y & 31)) & 1u) && rec.y < vmin) vmin = rec.y;
        if (tern && ((cur[rec.z >> 5] >> (rec.z & 31)) & 1u) && rec.z < vmin) vmin = rec.z;
        if (vmin != 0xFFFFFFFFu) run(vmin, r);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    uint32_t* t = cur; cur = nxt; nxt = t;
  }
  __syncthreads();

  if (PCP_ABLATE & 2048) tph[3] = wall_clock64();
  // ---- phase 3: status.  True iff no propagator is left that is not entailed (store.rs:250-256) -------------------------------
  const bool failed = misc[S_FAIL] != 0;
  if (!failed) {
    if constexpr (IMPLICIT) {
      const SetDom dm{bits, bnd, a.m.const_val, V, sw, a.base, nxt, misc, &narrow};
      for (uint32_t w = wv; w < words; w += nwv) {
        if (__builtin_amdgcn_readfirstlane(__hip_atomic_load(&misc[S_OPEN], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))) break;
        const uint32_t r = (w << 6) + lane;
        bool open_rec = false;
        if (r < P) open_rec = !eval_set(a.m.recs[r], dm, true);  // at the fixpoint the filters are no-ops: only is_subsumed()
        if (__ballot(open_rec) != 0 && lane == 0) atomicOr(&misc[S_OPEN], 1u);
      }
    } else {
      uint32_t cnt = 0;
      for (uint32_t w = tid; w < words; w += nth) cnt += (uint32_t)__popcll(live_row[w]);
      if (cnt) atomicOr(&misc[S_OPEN], 1u);
    }
  }
  // counters
  for (int o = 32; o > 0; o >>= 1) { narrow += __shfl_down(narrow, o); steps2 += __shfl_down(steps2, o); steps3 += __shfl_down(steps3, o); ev_only += __shfl_down(ev_only, o); }
  if (lane == 0) {
    if (narrow) atomicAdd(&misc[S_NARROW], narrow);
    if (ev_only) atomicAdd(reinterpret_cast<unsigned long long*>(&misc[S_EVAL]), (unsigned long long)ev_only);
    if (steps2) atomicAdd(reinterpret_cast<unsigned long long*>(&misc[S_STEPS2]), (unsigned long long)steps2);
    if (steps3) atomicAdd(reinterpret_cast<unsigned long long*>(&misc[S_STEPS3]), (unsigned long long)steps3);
  }
  __syncthreads();

  if (PCP_ABLATE & 2048) tph[4] = wall_clock64();
  // ---- phase 4: write back ------------------------------------------------------------------------------------------------
  {
    uint64_t* dst = a.bits_out + (size_t)node * V * sw;
    const uint32_t nwords = V * sw;
    if (!(nwords & 1u) && !((size_t)dst & 15)) {
      const uint4* s4 = reinterpret_cast<const uint4*>(bits);
      uint4* d4 = reinterpret_cast<uint4*>(dst);
      for (uint32_t i = tid; i < nwords / 2; i += nth) d4[i] = s4[i];
    } else {
      for (uint32_t i = tid; i < nwords; i += nth) dst[i] = bits[i];
    }
    for (uint32_t v = tid; v < V; v += nth) {
      const int2 b = bnd[v];
      a.lb_out[(size_t)node * V + v] = b.x;
      a.ub_out[(size_t)node * V + v] = b.y;
    }
  }
  if (tid == 0) {
    a.status[node] = failed ? (uint8_t)PCP_FALSE : (misc[S_OPEN] ? (uint8_t)PCP_UNKNOWN : (uint8_t)PCP_TRUE);
    const unsigned long long s2 = *reinterpret_cast<unsigned long long*>(&misc[S_STEPS2]);
    const unsigned long long s3 = *reinterpret_cast<unsigned long long*>(&misc[S_STEPS3]);
    if (s2) atomicAdd((unsigned long long*)&st_slot->steps, s2);
    if (s3) atomicAdd((unsigned long long*)&st_slot->steps3, s3);
    // evaluated = the pairs that were looked at: everything counted as a step except the bulk sweep's credit, plus its own few
    const unsigned long long evo = *reinterpret_cast<unsigned long long*>(&misc[S_EVAL]);
    const unsigned long long looked = s2 + s3 - (misc[S_LIVE] ? (unsigned long long)P : 0ull) + evo;
    if (looked) { atomicAdd((unsigned long long*)&st_slot->evaluated, looked); atomicAdd((unsigned long long*)&st_slot->full_evals, looked); }
    if (misc[S_NARROW]) atomicAdd((unsigned long long*)&st_slot->narrowings, (unsigned long long)misc[S_NARROW]);
    atomicAdd((unsigned long long*)&st_slot->waves, (unsigned long long)(1 + misc[S_WAVES]));
    atomicAdd((unsigned long long*)&st_slot->nodes, 1ull);
    if (failed) atomicAdd((unsigned long long*)&st_slot->failed_nodes, 1ull);
  }
  if (PCP_ABLATE & 2048) {  // staging / sweep / rounds / status / write-back ticks, summed over the nodes
    __syncthreads();
    if (tid == 0) {
      tph[5] = wall_clock64();
      atomicAdd((unsigned long long*)&st_slot->steps3, tph[1] - tph[0]);
      atomicAdd((unsigned long long*)&st_slot->narrowings, tph[2] - tph[1]);
      atomicAdd((unsigned long long*)&st_slot->failed_nodes, tph[3] - tph[2]);
      atomicAdd((unsigned long long*)&st_slot->waves, tph[4] - tph[3]);
      atomicAdd((unsigned long long*)&st_slot->evaluated, tph[5] - tph[4]);
    }
  }
}

// `active` rows of implicit set-mode nodes on request: bit r = record r is not entailed under the final sets.
__global__ void __launch_bounds__(kSetThreads) set_derive_active_kernel(const SetArgs a, uint64_t* live) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t tid = threadIdx.x, nth = blockDim.x, lane = tid & 63;
  const uint32_t wv = tid >> 6, nwv = nth >> 6;
  const uint32_t V = a.m.n_vars, S = a.m.n_slots, sw = a.set_words, P = a.m.n_recs, words = (P + 63) >> 6;
  const SetCarve cv = set_carve(V, S, sw, a.list_cap);
  unsigned long long* bits = reinterpret_cast<unsigned long long*>(smem + cv.bits);
  int2* bnd = reinterpret_cast<int2*>(smem + cv.bnd);
  uint32_t* misc = reinterpret_cast<uint32_t*>(smem + cv.misc);
  uint32_t* scratch = reinterpret_cast<uint32_t*>(smem + cv.chg_a);
  const uint32_t node = blockIdx.x;
  if (tid < 32) misc[tid] = 0;
  const uint64_t* src = a.bits_out + (size_t)node * V * sw;
  for (size_t i = tid; i < (size_t)V * sw; i += nth) bits[i] = src[i];
  __syncthreads();
  for (uint32_t v = tid; v < V; v += nth) bnd[v] = scan_bounds(bits + (size_t)v * sw, sw, a.base);
  __syncthreads();
  uint32_t narrow = 0;
  const SetDom dm{bits, bnd, a.m.const_val, V, sw, a.base, scratch, misc, &narrow};
  for (uint32_t w = wv; w < words; w += nwv) {
    const uint32_t r = (w << 6) + lane;
    bool on = false;
    if (r < P) on = !eval_set(a.m.recs[r], dm, true);
    const uint64_t word = __ballot(on);
    if (lane == 0) live[(size_t)node * words + w] = word;
  }
}

// ------------------------------------------------------------------------------------------------
// The search loop over FDSpace for stores of records, ONE TREE PER WORKGROUP (pcp_dfs_forest_device_set / _set_enum / _set_bnb): trail_dfs
// (pcp_setdfs.hpp: the loop, the trail, Enumerate and branch and bound) run by a WorkgroupTeam over a RecordNode.  Per node the HBM traffic
// is the trail (a few KB after an assignment, a few bytes otherwise) instead of the 125 KB-per-node rows of the batched search
// (pcp_propagate_device + pcp_branch_device_set).  Several trees = the subtrees of an open-node frontier, each on its CU.
// ------------------------------------------------------------------------------------------------
struct SetDfsCarve { SetCarve c; size_t touched, adjo, total; };

__host__ __device__ inline SetDfsCarve set_dfs_carve(uint32_t V, uint32_t S, uint32_t sw, uint32_t cap) {
  SetDfsCarve d;
  d.c = set_carve(V, S, sw, cap);
  d.touched = d.c.total;
  d.adjo = (d.touched + ((size_t)(S + 31) / 32) * 4 + 15) & ~(size_t)15;   // a copy of adj_off[V + 1]: no global load in a node's chains for it
  d.total = (d.adjo + ((size_t)V + 1) * 4 + 15) & ~(size_t)15;
  return d;
}

// A node of the records forest: setfix_kernel's propagation on a trailed node.  At a fixpoint every propagator is a no-op until one of its
// variables changes, so a child runs the changed-variable lists from its branched variable alone (two changed masks, cur and nxt, swapped
// every round); a root (pending == kDfsFull) runs the sweep of setfix_kernel first.
template <bool BNB>
struct RecordNode {
  using DM = SetDomT<true>;
  const SetDfsArgs& a;
  const WorkgroupTeam& team;
  unsigned long long* bits;
  int2* bnd;
  uint32_t *cur, *nxt, *list_id, *list_off, *list_deg, *misc, *touched, *adjo;
  uint4* trail;
  uint32_t mask_words;
  bool neq_only, use_pay;
  uint32_t narrow = 0;
  uint64_t ev = 0;
  unsigned long long key = ~0ull;

  __device__ __forceinline__ RecordNode(const SetDfsArgs& a_, const WorkgroupTeam& team_, unsigned char* smem, const SetDfsCarve& dcv, uint32_t t)
      : a(a_), team(team_),
        bits(reinterpret_cast<unsigned long long*>(smem + dcv.c.bits)), bnd(reinterpret_cast<int2*>(smem + dcv.c.bnd)),
        cur(reinterpret_cast<uint32_t*>(smem + dcv.c.chg_a)), nxt(reinterpret_cast<uint32_t*>(smem + dcv.c.chg_b)),
        list_id(reinterpret_cast<uint32_t*>(smem + dcv.c.list_id)), list_off(reinterpret_cast<uint32_t*>(smem + dcv.c.list_off)),
        list_deg(reinterpret_cast<uint32_t*>(smem + dcv.c.list_deg)), misc(reinterpret_cast<uint32_t*>(smem + dcv.c.misc)),
        touched(reinterpret_cast<uint32_t*>(smem + dcv.touched)), adjo(reinterpret_cast<uint32_t*>(smem + dcv.adjo)),
        trail(a_.trail + (size_t)t * a_.trail_cap), mask_words((a_.m.n_slots + 31) >> 5),
        neq_only(a_.m.uniform_kind == PCP_NEQ && a_.m.n_slots == a_.m.n_vars), use_pay(a_.m.adjp != nullptr && !a_.m.has_ternary) {}

  __device__ __forceinline__ uint32_t* mark_mask() const { return cur; }
  __device__ __forceinline__ DM dom(uint32_t* chg) { return DM{bits, bnd, a.m.const_val, a.m.n_vars, a.set_words, a.base, chg, misc, &narrow, trail, &misc[S_TRAILLEN], a.trail_cap}; }
  // a record as seen from variable v's list, entry idx: binary models rebuild it from the 8-byte adjacency payload (one coalesced load
  // instead of an index load and the gather that depends on it)
  __device__ __forceinline__ Rec rec_at(uint32_t v, uint32_t idx) const {
    if (use_pay) {
      const uint2 q = a.m.adjp[idx];
      const uint32_t other = q.x & kSlotMask, kind = (q.x >> 28) & 7u;
      const bool is_y = (q.x >> 31) != 0;
      Rec rc;
      rc.xk = (is_y ? other : v) | (kind << 28); rc.y = is_y ? v : other; rc.z = 0; rc.d = (int32_t)q.y;
      return rc;
    }
    return a.m.recs[a.m.adj[idx]];
  }

  __device__ __forceinline__ void load(const unsigned long long* gbits) {
    const uint32_t tid = team.rank, nth = team.size, V = a.m.n_vars;
    if (tid < 32) misc[tid] = 0;
    for (uint32_t i = tid; i < mask_words; i += nth) { cur[i] = 0; nxt[i] = 0; touched[i] = 0; }
    for (uint32_t v = tid; v <= V; v += nth) adjo[v] = a.m.adj_off[v];
    copy_node(team, bits, gbits, V * a.set_words);
    team.sync();
  }
  // launch start: the bounds of every variable; a node persisted by the launch before marks its pending variable again
  __device__ __forceinline__ void begin(uint32_t pending) {
    const uint32_t tid = team.rank, V = a.m.n_vars, sw = a.set_words;
    for (uint32_t v = tid; v < V; v += team.size) {
      const int2 b = scan_bounds(bits + (size_t)v * sw, sw, a.base);
      bnd[v] = b;
      if (b.x > b.y) atomicOr(&misc[S_FAIL], 1u);
    }
    if (pending != kDfsFull && tid == 0) cur[pending >> 5] = 1u << (pending & 31u);
    if constexpr (BNB) {
      // a persisted node was folded when it was entered, and that fold's mark went with the launch: the objective is marked again
      // (a variable marked without need only runs records that are no-ops at a fixpoint)
      if (pending != kDfsFull && tid == 0) cur[a.obj_var >> 5] |= 1u << (a.obj_var & 31u);
    }
    team.sync();
  }
  // after the fold of launch start: the sweep of a root reads bnd before the round loop scans anything, so the objective's bounds are
  // taken again here
  __device__ __forceinline__ void begun() {
    if constexpr (BNB) {
      if (team.leader()) {
        const int2 b = scan_bounds(bits + (size_t)a.obj_var * a.set_words, a.set_words, a.base);
        bnd[a.obj_var] = b;
        if (b.x > b.y) misc[S_FAIL] = 1u;
      }
      team.sync();
    }
  }

  __device__ __forceinline__ bool propagate(uint32_t pending) {
    const uint32_t tid = team.rank, nth = team.size, V = a.m.n_vars, sw = a.set_words, C = a.list_cap, P = a.m.n_recs;
    if (pending == kDfsFull && !misc[S_FAIL]) {
      const DM dm = dom(cur);
      bool bulk = false;
      if (neq_only) {  // the lists of the assigned variables stand for the whole sweep (see setfix_kernel)
        if (tid == 0) misc[S_NSING] = 0;
        team.sync();
        for (uint32_t v = tid; v < V; v += nth) {
          const int2 b = bnd[v];
          if (b.x == b.y) { const uint32_t pos = atomicAdd(&misc[S_NSING], 1u); if (pos < C) list_id[pos] = v; }
        }
        team.sync();
        const uint32_t ns = misc[S_NSING];
        bulk = ns <= C;
        if (bulk)
          for (uint32_t e = 0; e < ns; ++e) {
            const uint32_t v = list_id[e], o0 = adjo[v], o1 = adjo[v + 1];
            for (uint32_t i = o0 + tid; i < o1; i += nth) { (void)eval_set(rec_at(v, i), dm, false); ++ev; }
          }
      }
      if (!bulk)
        for (uint32_t r = tid; r < P; r += nth) { (void)eval_set(a.m.recs[r], dm, false); ++ev; }
      team.sync();
    }
    bool runaway = false;
    for (uint32_t round = 0;; ++round) {
      if (round >= (1u << 22)) { runaway = true; break; }  // (a round that runs narrows something: the cap only makes a runaway impossible)
      const uint32_t m_total = (round & 1u) ? S_TOTAL2 : S_TOTAL;
      for (uint32_t v = tid; v < V; v += nth) {
        if (!((cur[v >> 5] >> (v & 31)) & 1u)) continue;
        const int2 b = scan_bounds(bits + (size_t)v * sw, sw, a.base);
        bnd[v] = b;
        if (b.x > b.y) atomicOr(&misc[S_FAIL], 1u);
      }
      team.sync();
      for (uint32_t w = tid; w < mask_words; w += nth) {
        if (round) nxt[w] = 0;
        uint32_t bitsw = cur[w];
        if (!bitsw) continue;
        uint32_t dropped = 0;
        while (bitsw) {
          const uint32_t v = (w << 5) + __builtin_ctz(bitsw);
          bitsw &= bitsw - 1;
          if (v < V && neq_only) { const int2 b = bnd[v]; if (b.x != b.y) { dropped |= 1u << (v & 31); continue; } }
          const uint32_t pos = atomicAdd(&misc[m_total], 1u);
          if (pos < C) {
            const uint32_t o0 = (v < V) ? adjo[v] : 0u, o1 = (v < V) ? adjo[v + 1] : 0u;
            list_id[pos] = v; list_off[pos] = o0; list_deg[pos] = o1 - o0;
          }
        }
        if (dropped) cur[w] &= ~dropped;
      }
      team.sync();
      const uint32_t total = misc[m_total];
      if (total == 0 || misc[S_FAIL]) break;
      if (tid == 0) misc[(round & 1u) ? S_TOTAL : S_TOTAL2] = 0;
      const DM dm = dom(nxt);
      auto run = [&](uint32_t v, const Rec rec) {  // FIFO dedup as in setfix_kernel: the lowest changed variable of a record runs it
        const uint32_t x = rec.xk & kSlotMask;
        const bool tern = (rec.xk >> 28) > PCP_LT;
        if (x < v && ((cur[x >> 5] >> (x & 31)) & 1u)) return;
        if (rec.y < v && ((cur[rec.y >> 5] >> (rec.y & 31)) & 1u)) return;
        if (tern && rec.z < v && ((cur[rec.z >> 5] >> (rec.z & 31)) & 1u)) return;
        ++ev;
        (void)eval_set(rec, dm, false);
      };
      if (total <= C) {
        for (uint32_t e = 0; e < total; ++e) {
          const uint32_t v = list_id[e], deg = list_deg[e], off = list_off[e];
          for (uint32_t i = tid; i < deg; i += nth) run(v, rec_at(v, off + i));
        }
      } else {
        for (uint32_t r = tid; r < P; r += nth) {
          const Rec rec = a.m.recs[r];
          const uint32_t x = rec.xk & kSlotMask;
          const bool tern = (rec.xk >> 28) > PCP_LT;
          uint32_t vmin = 0xFFFFFFFFu;
          if ((cur[x >> 5] >> (x & 31)) & 1u) vmin = x;
          if (((cur[rec.y >> 5] >> (rec.y & 31)) & 1u) && rec.y < vmin) vmin = rec.y;
          if (tern && ((cur[rec.z >> 5] >> (rec.z & 31)) & 1u) && rec.z < vmin) vmin = rec.z;
          if (vmin != 0xFFFFFFFFu) run(vmin, rec);
        }
      }
      team.sync();
      uint32_t* sw_ = cur; cur = nxt; nxt = sw_;
    }
    team.sync();
    return runaway;
  }

  // status (store.rs:250-256): failed / every propagator entailed / open.  The candidate for branching first (first_smallest_var): an open
  // node almost always has an open record in that variable's list, while the table's first records belong to the variables a dive
  // assigned first and are all entailed.  Only when the list holds no open record is the whole table scanned (exact either way).  The
  // minimum across wavefronts goes through list_off, idle between rounds (16 x 8 bytes).
  __device__ __forceinline__ NodeStatus status() {
    const uint32_t lane = team.lane, wv = team.wave, P = a.m.n_recs, words = (P + 63) >> 6;
    const bool failed = misc[S_FAIL] != 0;
    key = ~0ull;
    if (!failed) {
      key = first_smallest_var(team, bits, a.m.n_vars, a.set_words, a.var_select);
      const DM dm = dom(nxt);
      if (key != ~0ull) {
        const uint32_t u = (uint32_t)key, o0 = adjo[u], o1 = adjo[u + 1];
        for (uint32_t i0 = o0 + wv * 64; i0 < o1; i0 += team.size) {
          if (__builtin_amdgcn_readfirstlane(__hip_atomic_load(&misc[S_OPEN], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))) break;
          bool open_rec = false;
          if (i0 + lane < o1) open_rec = !eval_set(rec_at(u, i0 + lane), dm, true);
          if (__ballot(open_rec) != 0 && lane == 0) atomicOr(&misc[S_OPEN], 1u);
        }
      }
      team.sync();
      if (!misc[S_OPEN]) {
        for (uint32_t w = wv; w < words; w += team.n_waves) {
          if (__builtin_amdgcn_readfirstlane(__hip_atomic_load(&misc[S_OPEN], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))) break;
          const uint32_t r = (w << 6) + lane;
          bool open_rec = false;
          if (r < P) open_rec = !eval_set(a.m.recs[r], dm, true);  // at the fixpoint the filters are no-ops: only is_subsumed()
          if (__ballot(open_rec) != 0 && lane == 0) atomicOr(&misc[S_OPEN], 1u);
        }
      }
    }
    team.sync();
    if (failed)  // (only a failed node leaves marks behind; its backtrack has barriers before anything is marked again)
      for (uint32_t i = team.rank; i < mask_words; i += team.size) { cur[i] = 0; nxt[i] = 0; }
    return NodeStatus{failed, misc[S_OPEN] != 0};
  }
  __device__ __forceinline__ unsigned long long branch_key() const { return key; }  // (status() needed it to probe the node)
  __device__ __forceinline__ void backtracking() {}  // (the levels and the trail were synchronised by the barriers of propagate() and status())
  __device__ __forceinline__ void backtracked() {}
  __device__ __forceinline__ void end_node() {
    if (team.leader()) { misc[S_OPEN] = 0; misc[S_TOTAL] = 0; misc[S_TOTAL2] = 0; }  // (a node's last round leaves its count behind)
  }
  __device__ __forceinline__ void flush_stats(pcp_stats* st_slot, unsigned long long c_nodes) {
    for (int o = 32; o > 0; o >>= 1) { narrow += __shfl_down(narrow, o); ev += __shfl_down(ev, o); }
    if (team.lane == 0) {
      if (narrow) atomicAdd((unsigned long long*)&st_slot->narrowings, (unsigned long long)narrow);
      if (ev) { atomicAdd((unsigned long long*)&st_slot->evaluated, (unsigned long long)ev); atomicAdd((unsigned long long*)&st_slot->full_evals, (unsigned long long)ev); }
    }
    // reference-equivalent steps: every propagator of every node once (init_scheduler) — the wake-ups are in `evaluated`
    if (team.leader()) atomicAdd((unsigned long long*)&st_slot->steps, c_nodes * (unsigned long long)a.m.n_recs);
  }
};

// ENUM, BNB, SINK: see trail_dfs.  The BNB = false instantiations carry no branch-and-bound code, the ENUM = false ones no value selector,
// the SINK = false ones no set solution sink.
template <bool ENUM, bool BNB, bool SINK>
__global__ void __launch_bounds__(kSetThreads) setdfs_kernel(const SetDfsArgs a, const SetSinkDev sink) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const SetDfsCarve dcv = set_dfs_carve(a.m.n_vars, a.m.n_slots, a.set_words, a.list_cap);
  const WorkgroupTeam team(reinterpret_cast<uint32_t*>(smem + dcv.c.misc), reinterpret_cast<unsigned long long*>(smem + dcv.c.list_off));
  RecordNode<BNB> node(a, team, smem, dcv, blockIdx.x);
  trail_dfs<ENUM, BNB, SINK>(a, sink, blockIdx.x, team, node);
}

// A finished tree takes over the OLDEST open right branch of a tree that still has some (the subtree nearest the donor's root: the
// largest it can give).  That node = the donor's current node with its trail undone down to the level's mark (the parent's fixpoint)
// and the right branch applied; it is built straight into the receiver's row.  The donor's level is marked as given (levels[..].w):
// its search loop undoes it like any other level and does not take the right branch.  Runs BETWEEN launches of setdfs_kernel.
// Under branch and bound (setdfs_kernel<.., true>) nothing changes here: the level's mark was taken at the parent's fixpoint, the parent's
// own fold lies below it on the trail, so the handed-over node is that fixpoint, fold included, plus the right branch; the receiver folds
// the incumbent of the moment into it at its next launch start and marks the objective changed, as for a node it persisted itself.
__global__ void __launch_bounds__(256) setdfs_split_kernel(const SetDfsArgs a, const uint32_t* __restrict__ pairs, uint32_t* __restrict__ done) {
  const uint32_t d = pairs[2 * blockIdx.x], r = pairs[2 * blockIdx.x + 1], tid = threadIdx.x, nth = blockDim.x;
  const uint32_t V = a.m.n_vars, sw = a.set_words;
  uint32_t* const td = a.tree + (size_t)d * 4;
  uint32_t* const tr = a.tree + (size_t)r * 4;
  const uint32_t n_levels = td[0], tlen = td[1], given = td[3] >> 8;
  const bool ok = !(td[3] & 1u) && (tr[3] & 1u) && given < n_levels && d != r;
  if (!ok) { if (tid == 0) done[blockIdx.x] = 0; return; }
  uint4* const lvp = a.levels + (size_t)d * a.level_cap + given;
  const uint4 lv = *lvp;
  const unsigned long long* src = reinterpret_cast<const unsigned long long*>(a.bits) + (size_t)d * V * sw;
  unsigned long long* dst = reinterpret_cast<unsigned long long*>(a.bits) + (size_t)r * V * sw;
  for (uint32_t i = tid; i < V * sw; i += nth) dst[i] = src[i];
  __syncthreads();
  const uint4* trail = a.trail + (size_t)d * a.trail_cap;
  for (uint32_t i = lv.z + tid; i < tlen; i += nth) {
    const uint4 e = trail[i];
    atomicOr(&dst[e.x], ((unsigned long long)e.w << 32) | e.z);
  }
  __syncthreads();
  // the right child, by the level's own distributor — x > val: the values up to val leave the variable's set (binary_split.rs:52-57);
  // x != val: val alone does (enumerate.rs:54-59)
  for (uint32_t k = tid; k < sw; k += nth) {
    const long long t = (long long)(int)lv.y - ((long long)a.base + 64ll * (long long)k);
    unsigned long long gone = t < 0 ? 0ull : (t >= 63 ? ~0ull : ((2ull << t) - 1ull));
    if (lv.w & kLevelEnum) gone = (t < 0 || t > 63) ? 0ull : (1ull << t);
    dst[(size_t)lv.x * sw + k] &= ~gone;
  }
  if (tid == 0) {
    lvp->w = lv.w | kLevelGiven;
    td[3] = (td[3] & 0xFFu) | ((given + 1) << 8);
    tr[0] = 0; tr[1] = 0; tr[2] = lv.x; tr[3] = 0;
    done[blockIdx.x] = 1;
  }
}

size_t lds_bytes_set_dfs(uint32_t n_vars, uint32_t n_slots, uint32_t set_words, uint32_t list_cap) {
  const SetDfsCarve c = set_dfs_carve(n_vars, n_slots, set_words, list_cap);
  return c.total <= 160 * 1024 ? c.total : 0;
}

template <bool ENUM, bool BNB, bool SINK>
static hipError_t launch_setdfs_as(const SetDfsArgs& a, const SetSinkDev& sink, size_t lds, hipStream_t stream) {
  hipError_t e;
  if (lds > 64 * 1024 && (e = hipFuncSetAttribute(reinterpret_cast<const void*>(setdfs_kernel<ENUM, BNB, SINK>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) != hipSuccess) return e;
  hipLaunchKernelGGL((setdfs_kernel<ENUM, BNB, SINK>), dim3(a.n_trees), dim3(kSetThreads), lds, stream, a, sink);
  return hipGetLastError();
}

hipError_t launch_setdfs(const SetDfsArgs& a, const SetSinkDev& sk, bool enumerate, bool bnb, hipStream_t stream) {
  const size_t lds = set_dfs_carve(a.m.n_vars, a.m.n_slots, a.set_words, a.list_cap).total;
  // the context's set solution sink (pcp_set_solution_sink_set); the branch-and-bound entry refuses it
  const bool sink = sk.bits != nullptr;
  if (sink && (bnb || !sk.count || !sk.capacity)) return hipErrorInvalidValue;
  if (bnb) return enumerate ? launch_setdfs_as<true, true, false>(a, sk, lds, stream) : launch_setdfs_as<false, true, false>(a, sk, lds, stream);
  if (sink) return enumerate ? launch_setdfs_as<true, false, true>(a, sk, lds, stream) : launch_setdfs_as<false, false, true>(a, sk, lds, stream);
  return enumerate ? launch_setdfs_as<true, false, false>(a, sk, lds, stream) : launch_setdfs_as<false, false, false>(a, sk, lds, stream);
}

hipError_t launch_setdfs_split(const SetDfsArgs& a, uint32_t n_pairs, const uint32_t* pairs, uint32_t* done, hipStream_t stream) {
  if (!n_pairs) return hipSuccess;
  hipLaunchKernelGGL(setdfs_split_kernel, dim3(n_pairs), dim3(256), 0, stream, a, pairs, done);
  return hipGetLastError();
}

hipError_t launch_setfix(const ModelDev& m, uint32_t n_nodes, uint32_t set_words, int32_t base, uint32_t list_cap, const uint64_t* bits_in,
                         uint64_t* bits_out, int32_t* lb_out, int32_t* ub_out, const uint64_t* live_in, uint64_t* live, uint8_t* status,
                         pcp_stats* stats, uint64_t* derive_into, hipStream_t stream) {
  SetArgs a{m, n_nodes, set_words, list_cap, base, bits_in, bits_out, lb_out, ub_out, live_in, live, status, stats};
  const size_t lds = set_carve(m.n_vars, m.n_slots, set_words, list_cap).total;
  hipError_t e;
  if (live) {
    if (lds > 64 * 1024 && (e = hipFuncSetAttribute(reinterpret_cast<const void*>(setfix_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) != hipSuccess) return e;
    hipLaunchKernelGGL(setfix_kernel<false>, dim3(n_nodes), dim3(kSetThreads), lds, stream, a);
  } else {
    if (lds > 64 * 1024 && (e = hipFuncSetAttribute(reinterpret_cast<const void*>(setfix_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) != hipSuccess) return e;
    hipLaunchKernelGGL(setfix_kernel<true>, dim3(n_nodes), dim3(kSetThreads), lds, stream, a);
  }
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (derive_into) {
    if (lds > 64 * 1024 && (e = hipFuncSetAttribute(reinterpret_cast<const void*>(set_derive_active_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) != hipSuccess) return e;
    hipLaunchKernelGGL(set_derive_active_kernel, dim3(n_nodes), dim3(kSetThreads), lds, stream, a, derive_into);
    e = hipGetLastError();
  }
  return e;
}

// ------------------------------------------------------------------------------------------------
// Brancher<FirstSmallestVar | InputOrder, MiddleVal, BinarySplit>::enter over FDSpace (search/branching/brancher.rs:52-71): the variable of
// minimal CARDINALITY > 1, first index (first_smallest_var.rs:30-39 uses Domain::size()) or, under var_select = PCP_VAR_INPUT_ORDER, the
// first variable of cardinality > 1 (input_order.rs:30-39), the value (lower + upper) / 2
// (middle_val.rs:25-27), children `x <= v` / `x > v` (binary_split.rs:46-57) folded into the variable's set.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) set_branch_kernel(uint32_t V, uint32_t sw, int32_t base, uint32_t words, const uint64_t* __restrict__ bits,
                                                         const int32_t* __restrict__ lb, const int32_t* __restrict__ ub,
                                                         const uint64_t* __restrict__ active, const uint32_t* __restrict__ child_base,
                                                         uint64_t* __restrict__ child_bits, uint64_t* __restrict__ child_active,
                                                         const uint32_t* __restrict__ counts, uint32_t reverse, uint32_t var_select) {
  const uint32_t node = blockIdx.x, tid = threadIdx.x, nth = blockDim.x;
  const uint32_t slot = child_base[node];
  if (slot == 0xFFFFFFFFu) return;
  const uint32_t rowL = reverse ? counts[0] - 1 - slot : slot;
  const uint32_t rowR = reverse ? rowL - 1 : slot + 1;
  __shared__ unsigned long long best[4];
  const uint64_t* pb = bits + (size_t)node * V * sw;
  const uint32_t size_mask = var_size_mask(var_select);  // (InputOrder: the first variable of cardinality > 1)
  unsigned long long key = ~0ull;
  for (uint32_t v = tid; v < V; v += nth) {
    unsigned long long size = 0;
    for (uint32_t k = 0; k < sw; ++k) size += (unsigned long long)__popcll(pb[(size_t)v * sw + k]);
    if (size > 1) key = min(key, var_key(size, v, size_mask));
  }
  for (int o = 32; o > 0; o >>= 1) key = min(key, (unsigned long long)__shfl_down(key, o));
  if ((tid & 63) == 0) best[tid >> 6] = key;
  __syncthreads();
  key = best[0];
  for (uint32_t w = 1; w < (nth >> 6); ++w) key = min(key, best[w]);
  const uint32_t var = key == ~0ull ? 0xFFFFFFFFu : (uint32_t)key;
  long long val = 0;
  if (var != 0xFFFFFFFFu) val = ((long long)lb[(size_t)node * V + var] + (long long)ub[(size_t)node * V + var]) / 2;
  uint64_t* b0 = child_bits + (size_t)rowL * V * sw;
  uint64_t* b1 = child_bits + (size_t)rowR * V * sw;
  for (size_t i = tid; i < (size_t)V * sw; i += nth) {
    const uint64_t w = pb[i];
    uint64_t le = ~0ull;  // the values <= val within this word
    if ((uint32_t)(i / sw) == var) {
      const long long t = val - ((long long)base + 64ll * (long long)(i % sw));
      le = t < 0 ? 0ull : (t >= 63 ? ~0ull : ((2ull << t) - 1ull));
      b0[i] = w & le;
      b1[i] = w & ~le;
    } else {
      b0[i] = w;
      b1[i] = w;
    }
  }
  if (active) {
    const uint64_t* pa = active + (size_t)node * words;
    uint64_t* a0 = child_active + (size_t)rowL * words;
    uint64_t* a1 = child_active + (size_t)rowR * words;
    for (uint32_t w = tid; w < words; w += nth) { const uint64_t x = pa[w]; a0[w] = x; a1[w] = x; }
  }
}

hipError_t launch_set_branch(uint32_t n_nodes, uint32_t n_vars, uint32_t set_words, int32_t base, uint32_t words, const uint64_t* bits, const int32_t* lb,
                             const int32_t* ub, const uint64_t* active, const uint8_t* status, uint64_t* child_bits, uint64_t* child_active,
                             uint32_t* child_base, uint32_t* counts, uint32_t reverse, uint32_t var_select, hipStream_t stream) {
  hipError_t e = launch_branch_scan(n_nodes, status, child_base, counts, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(set_branch_kernel, dim3(n_nodes), dim3(256), 0, stream, n_vars, set_words, base, words, bits, lb, ub, active, child_base, child_bits,
                     child_active, counts, reverse, var_select);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Brancher<FirstSmallestVar, MiddleVal | MinVal, Enumerate>::enter over FDSpace (search/branching/brancher.rs:52-71,
// search/branching/enumerate.rs:47-60): the variable of set_branch_kernel; the member of its set nearest to the selector's value
// (min_val.rs:25-27: lb; middle_val.rs:25-27: (lb + ub) / 2), the lower one first — the value itself whenever it is a member;
// children `x = v` (the set becomes {v}) and `x != v` (bit v cleared), rows as set_branch_kernel writes them.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) set_branch_enum_kernel(uint32_t V, uint32_t sw, int32_t base, uint32_t words, const uint64_t* __restrict__ bits,
                                                              const int32_t* __restrict__ lb, const int32_t* __restrict__ ub,
                                                              const uint64_t* __restrict__ active, const uint32_t* __restrict__ child_base,
                                                              uint32_t val_mode, uint64_t* __restrict__ child_bits, uint64_t* __restrict__ child_active,
                                                              uint32_t* __restrict__ counts, uint32_t reverse, uint32_t var_select) {
  const uint32_t node = blockIdx.x, tid = threadIdx.x, nth = blockDim.x;
  const uint32_t slot = child_base[node];
  if (slot == 0xFFFFFFFFu) return;
  const uint32_t rowL = reverse ? counts[0] - 1 - slot : slot;
  const uint32_t rowR = reverse ? rowL - 1 : slot + 1;
  __shared__ unsigned long long best[4], near[4];
  const uint64_t* pb = bits + (size_t)node * V * sw;
  const uint32_t size_mask = var_size_mask(var_select);  // (InputOrder: the first variable of cardinality > 1)
  unsigned long long key = ~0ull;
  for (uint32_t v = tid; v < V; v += nth) {
    unsigned long long size = 0;
    for (uint32_t k = 0; k < sw; ++k) size += (unsigned long long)__popcll(pb[(size_t)v * sw + k]);
    if (size > 1) key = min(key, var_key(size, v, size_mask));
  }
  for (int o = 32; o > 0; o >>= 1) key = min(key, (unsigned long long)__shfl_down(key, o));
  if ((tid & 63) == 0) best[tid >> 6] = key;
  __syncthreads();
  key = best[0];
  for (uint32_t w = 1; w < (nth >> 6); ++w) key = min(key, best[w]);
  if (key == ~0ull) {
    // Unknown, yet no variable with more than one value: the reference panics here (first_smallest_var.rs:36); the rows stay unwritten
    if (tid == 0) atomicMax(&counts[6], 3u);
    return;
  }
  const uint32_t var = (uint32_t)key;
  const long long lo = lb[(size_t)node * V + var], hi = ub[(size_t)node * V + var];
  const long long m = val_mode == PCP_VAL_MIN ? lo : (lo + hi) / 2;
  unsigned long long nk = ~0ull;
  for (uint32_t k = tid; k < sw; k += nth) nk = min(nk, nearest_member_key(pb[(size_t)var * sw + k], (long long)base + 64ll * (long long)k, m));
  for (int o = 32; o > 0; o >>= 1) nk = min(nk, (unsigned long long)__shfl_down(nk, o));
  if ((tid & 63) == 0) near[tid >> 6] = nk;
  __syncthreads();
  nk = near[0];
  for (uint32_t w = 1; w < (nth >> 6); ++w) nk = min(nk, near[w]);
  const long long vbit = nearest_member_value(nk, m) - (long long)base;  // (the set has two members or more: one was found)
  const uint32_t vword = (uint32_t)(vbit >> 6);
  const uint64_t one = 1ull << (vbit & 63);
  uint64_t* b0 = child_bits + (size_t)rowL * V * sw;
  uint64_t* b1 = child_bits + (size_t)rowR * V * sw;
  for (size_t i = tid; i < (size_t)V * sw; i += nth) {
    const uint64_t w = pb[i];
    if ((uint32_t)(i / sw) == var) {
      const bool here = (uint32_t)(i % sw) == vword;
      b0[i] = here ? one : 0ull;    // x = v
      b1[i] = here ? w & ~one : w;  // x != v
    } else {
      b0[i] = w;
      b1[i] = w;
    }
  }
  if (active) {
    const uint64_t* pa = active + (size_t)node * words;
    uint64_t* a0 = child_active + (size_t)rowL * words;
    uint64_t* a1 = child_active + (size_t)rowR * words;
    for (uint32_t w = tid; w < words; w += nth) { const uint64_t x = pa[w]; a0[w] = x; a1[w] = x; }
  }
}

hipError_t launch_set_branch_enum(uint32_t n_nodes, uint32_t n_vars, uint32_t set_words, int32_t base, uint32_t words, const uint64_t* bits, const int32_t* lb,
                                  const int32_t* ub, const uint64_t* active, const uint8_t* status, uint32_t val, uint64_t* child_bits, uint64_t* child_active,
                                  uint32_t* child_base, uint32_t* counts, uint32_t reverse, uint32_t var_select, hipStream_t stream) {
  hipError_t e = launch_branch_scan(n_nodes, status, child_base, counts, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(set_branch_enum_kernel, dim3(n_nodes), dim3(256), 0, stream, n_vars, set_words, base, words, bits, lb, ub, active, child_base, val,
                     child_bits, child_active, counts, reverse, var_select);
  return hipGetLastError();
}

}  // namespace pcp
