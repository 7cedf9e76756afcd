// pcp_internal.h — shared between the C-ABI host code (pcp_api.hip) and the gfx950 kernels (pcp_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pcp_hip.h"
#include "pcp_tables.h"  // Rec, Rec8, WordDesc, GroupDesc and the limits of the model tables

namespace pcp {

// term::Sum views (term/sum.rs:56-92): pseudo-slots [first, first + count) whose domain is the interval sum of their member
// variables, computed on demand; an update through a Sum of several variables never narrows, it only has to overlap.
struct SumTab {
  const uint32_t* off;  // [count + 1] into mem
  const uint32_t* mem;  // member variable indices
  uint32_t first;       // first sum slot (= n_vars)
  uint32_t count;       // 0 = the model has no Sum view
  const int32_t* mul_off;  // XEqYMulZ records: (dx, dy, dz) Addition offsets of the three operands, indexed by the record's `d`
};

struct ModelDev {
  const Rec* recs;          // [n_recs]
  const Rec8* recs8;        // [n_recs] or null when the model is not compactable
  const WordDesc* wdesc;    // [ceil(n_recs/64)] word descriptors, or null
  const GroupDesc* gdesc;   // [ceil(n_recs/4096)] group descriptors (with wdesc), or null
  const uint32_t* adj_off;  // [n_vars + 1]  CSR var -> incident record ids (constants have no adjacency)
  const uint32_t* adj;      // [adj_off[n_vars]]
  const uint2* adjp;        // [adj_off[n_vars]] payload of each adjacency entry of a binary-only model, or null:
                            //   .x = the record's OTHER operand slot | kind << 28 | (this variable is the record's y) << 31,  .y = d
                            // — the wake-up rounds rebuild the record from it instead of gathering 16 bytes per entry
  const int32_t* const_val; // [n_slots - n_vars]
  uint32_t n_recs;
  uint32_t n_vars;
  uint32_t n_slots;  // n_vars + number of interned constants
  uint32_t has_ternary;
  uint32_t uniform_kind;  // the kind shared by ALL records when that is NEQ or LT, else 0xFFFFFFFF (the sweep then classifies each chunk)
  uint32_t max_deg;       // longest adjacency list of a variable
  SumTab sums;            // Sum views; with count > 0 every record takes the generic path (no compact stream, no payloads)
};

// Per-launch arguments of the fixpoint kernel.
struct LaunchArgs {
  ModelDev m;
  uint32_t n_nodes;
  uint32_t nodes_per_block;  // B: nodes whose domains one workgroup keeps in LDS (team == 1)
  uint32_t team;             // G: workgroups cooperating on ONE node (nodes_per_block == 1 when team > 1)
  uint32_t list_cap;         // capacity of the per-round changed-(node,var) list in LDS
  uint32_t global_dom;       // 1 = domains stay in lb_out/ub_out (HBM/L2), for variable stores larger than LDS
  uint32_t word_level;       // packed tiles only: 1 = sweep by word groups with the level -1 range test (needs m.wdesc),
                             //     2 = the same with maximum tables as well (the model has XLessY words)
  uint32_t packed;           // 1 = 16-bit packed LDS domains (every bound within +-kPackedMax); tiles that do not fit mark
                             //     their nodes kStatusRetry, raise *retry_flag to `epoch` and leave the outputs untouched
  uint32_t adj_cache;        // 1 = (n_vars + 1) words of LDS behind the carve hold a copy of m.adj_off
  uint32_t solo;             // 1 = a round with a single changed variable re-runs its records in place and jumps over forbidden values (rounds, c0)
  uint32_t* violation;       // sticky device word (pcp_stats_read reports and clears it): a node was refused with PCP_STATUS_HULL
  uint32_t dom10;            // global_dom launches only: 1 = the node's domains sit in LDS after all, as 10-bit (lb - lo, ub - lo) cells, three
                             //     per u64 (a declared hull of at most 1024 values: 50 000 variables = 130 KB), behind the carve
  int32_t dom10_lo;          // the hull's lower bound
  uint32_t only_marked;      // 1 = second launch of a packed call: run only tiles whose nodes carry kStatusRetry
  uint32_t epoch;            // launch stamp compared with *retry_flag
  uint32_t* retry_flag;      // device word of the context
  const uint32_t* sp_ptr;    // device-side DFS (pcp_dfs_device): the node to run is row *sp_ptr - 1 of the buffers below (nothing to do
                             //     when *sp_ptr == 0 or *stop_ptr != 0); null = rows [0, n_nodes)
  const uint32_t* stop_ptr;
  const int32_t* lb_in;
  const int32_t* ub_in;
  int32_t* lb_out;
  int32_t* ub_out;
  const uint64_t* live_in;  // [n_nodes][words] or null = all live
  uint64_t* live;           // [n_nodes][words] working + output live mask; null = IMPLICIT: no live rows at all, every record is
                            //     taken as live and the status comes from an entailment scan of the final domains
  uint8_t* status;
  pcp_stats* stats;         // device counters
  // team mode scratch (per node): arrival ticket, merged changed mask, remaining counter, fail flag
  uint32_t* team_ticket;    // [n_nodes]
  uint32_t* team_chg;       // [n_nodes][chg_words]
  uint32_t* team_remaining; // [n_nodes]
  uint32_t* team_fail;      // [n_nodes]
  uint64_t* team_counters;  // [n_nodes][kTeamCounters] steps, steps3, narrowings, evaluated, full_evals (merged by the tail block)
};

constexpr uint32_t kTeamCounters = 6;
constexpr uint32_t kStatSlots = 64;  // the device counters are striped over this many pcp_stats structs (workgroup b adds to slot b % kStatSlots;
                                      // pcp_stats_read sums them): same-address device atomics serialise at ~12 ns each, chip-wide
constexpr uint8_t kStatusRetry = 0xFE;  // internal: never visible to the caller (the second launch overwrites it)

struct LaunchPlan {
  uint32_t grid;
  uint32_t block;
  size_t lds_bytes;
};

// Computes the dynamic-LDS footprint for (n_slots, B, list_cap); returns 0 if it cannot fit.
size_t lds_bytes_for(uint32_t n_slots, uint32_t nodes_per_block, uint32_t list_cap, uint32_t block, bool packed = false, uint32_t word_level = 0);
size_t lds_bytes_global(uint32_t n_vars, uint32_t n_slots, uint32_t list_cap);
inline size_t dom10_bytes(uint32_t n_vars) { return ((((size_t)n_vars + 2) / 3) * 8 + 15) & ~(size_t)15; }

hipError_t launch_fixpoint(const LaunchArgs& a, const LaunchPlan& p, hipStream_t stream);

// Grouped models (Conjunction / Distinct units): unit-level `active` rows <-> record-level live rows.
hipError_t launch_expand_units(const uint32_t* rec_unit, uint32_t n_recs, uint32_t unit_words, const uint64_t* active_in, uint64_t* live,
                               uint32_t n_nodes, hipStream_t stream);
hipError_t launch_contract_units(const uint32_t* unit_first, uint32_t n_units, uint32_t n_recs, const uint64_t* live, uint64_t* active_out,
                                 uint32_t n_nodes, hipStream_t stream);

// Implicit-active nodes: record-level live rows from the final domains (live bit = the record is not entailed).
hipError_t launch_derive_active(const ModelDev& m, const int32_t* lb, const int32_t* ub, uint64_t* live, uint32_t n_nodes, hipStream_t stream);

// Set mode (pcp_set.hip): IntervalSet<i32> domains as bitsets, one workgroup per node.  live == nullptr: implicit-active nodes;
// derive_into != nullptr: record-level live rows materialised from the final sets afterwards.
size_t lds_bytes_set(uint32_t n_vars, uint32_t n_slots, uint32_t set_words, uint32_t list_cap);
hipError_t launch_setfix(const ModelDev& m, uint32_t n_nodes, uint32_t set_words, int32_t base, uint32_t list_cap, const uint64_t* bits_in,
                         uint64_t* bits_out, int32_t* lb_out, int32_t* ub_out, const uint64_t* live_in, uint64_t* live, uint8_t* status,
                         pcp_stats* stats, uint64_t* derive_into, hipStream_t stream);

// The set solution sink of a context (pcp_set_solution_sink_set): an append buffer of whole nodes — n_vars x set_words 64-bit words, the
// layout of a pcp_forest_state.bits row — every tree of a set-mode forest writes its solutions into.  A solution draws a ticket from *count
// BEFORE it is counted; a ticket >= capacity hands the node back to the caller (error kSetDfsSinkFull, the contract of error 1 in
// trail_dfs).  The SINK = false instantiations never read the struct.  It is a kernel argument OF ITS OWN behind SetDfsArgs /
// SetFormDfsArgs, not a member of SetDfsArgs: that struct is the first member of SetFormDfsArgs, and growing it moved the formula fields
// behind it, which changed the SGPR spill counts of setformdfs_kernel's existing branch-and-bound instantiations; appended behind both
// structs, every argument that existed keeps its offset and every existing instantiation its figures (profiles/set_forest_sink_resource_usage.txt).
struct SetSinkDev {
  uint64_t* bits;     // [capacity][n_vars][set_words]
  uint32_t* tree;     // [capacity] or null: the tree that wrote the row
  uint32_t* count;    // tickets drawn since the caller last zeroed it
  uint32_t capacity;
};
constexpr uint32_t kSetDfsSinkFull = 6;  // counters[t][3]: the sink was full — the node stays the tree's current node, at its fixpoint and uncounted

// Set mode, the search loop on the device: one tree per workgroup, the current node in LDS, an undo trail in HBM (pcp_set.hip).
struct SetDfsArgs {
  ModelDev m;
  uint32_t set_words, list_cap;
  int32_t base;
  uint32_t n_trees, level_cap, trail_cap, n_steps, stop_on_solution;
  unsigned long long node_limit;
  uint64_t* bits;                 // [n_trees][n_vars][set_words]: each tree's current node
  uint32_t* tree;                 // [n_trees][4]: levels, trail length, pending variable, finished
  uint4* levels;                  // [n_trees][level_cap]: (variable, value, trail mark, kLevelGiven | kLevelEnum)
  uint4* trail;                   // [n_trees][trail_cap]: (word index, variable, removed bits lo, hi)
  unsigned long long* counters;   // [n_trees][4]: nodes, solutions, failed, error
  unsigned long long* total_nodes;
  uint32_t* stop;
  int32_t* first_solution;
  uint32_t* solution_flag;
  pcp_stats* stats;
  uint32_t val_mode;              // the Enumerate loop only: PCP_VAL_MIDDLE / PCP_VAL_MIN
  uint32_t var_select;            // PCP_VAR_FIRST_SMALLEST / PCP_VAR_INPUT_ORDER (option "var_select")
  // branch and bound only (setdfs_kernel<.., true>, pcp_dfs_forest_device_set_bnb)
  uint32_t obj_var, obj_mode;     // the objective variable, PCP_MINIMIZE / PCP_MAXIMIZE
  int32_t* obj_best;              // device int32[1]: the forest's incumbent
  int32_t* tree_best;             // [n_trees]: the value of each tree's last solution
  int32_t* tree_row;              // [n_trees][n_vars] or null: its lower bounds
};
// a level's flags (levels[..].w): its right branch went to another tree (setdfs_split_kernel); its distributor is Enumerate (x = v, then
// x != v) instead of BinarySplit (x <= v, then x > v)
constexpr uint32_t kLevelGiven = 1u, kLevelEnum = 2u;
constexpr uint32_t kDfsFull = 0xFFFFFFFFu;  // tree[..][2]: the current node has not been propagated at all (PCP_DFS_FULL)
constexpr uint32_t kDfsChunk = 8;            // nodes a tree reserves from the forest's counter at a time
size_t lds_bytes_set_dfs(uint32_t n_vars, uint32_t n_slots, uint32_t set_words, uint32_t list_cap);
// (sink.bits != null: the instantiation that appends every solution to the set sink; never together with bnb)
hipError_t launch_setdfs(const SetDfsArgs& a, const SetSinkDev& sink, bool enumerate, bool bnb, hipStream_t stream);
hipError_t launch_setdfs_split(const SetDfsArgs& a, uint32_t n_pairs, const uint32_t* pairs, uint32_t* done, hipStream_t stream);

// Interval forests, between two launches (pcp_steal.hip, pcp_dfs_forest_steal): idle trees take the bottom row of trees with two or more
// open nodes.  The state of pcp_dfs_state / pcp_forest_excl as the steal reads it; the store is not looked at.
struct StealArgs {
  int32_t* lb;          // [n_trees][capacity][n_vars]
  int32_t* ub;
  uint32_t* sp;         // [n_trees]
  uint32_t* dirty;      // [n_trees][capacity] or null
  pcp_excl* path;       // [n_trees][path_capacity]; null without exclusions, or with path_capacity == 0
  uint32_t* row_base;   // [n_trees][capacity]; null = no exclusion state (BinarySplit forests)
  pcp_excl* row_excl;   // [n_trees][capacity], with row_base
  uint32_t n_trees, capacity, n_vars, path_capacity, n_pairs;
  uint32_t col_slices;  // set by the launcher: blocks per pair that move columns
};
// pairs: n_pairs x (donor, receiver); done[i] = 1 where pair i was valid on the state the call found and was carried out, else 0.
hipError_t launch_forest_steal(const StealArgs& a, const uint32_t* pairs, uint32_t* done, hipStream_t stream);

hipError_t launch_branch_scan(uint32_t n_nodes, const uint8_t* status, uint32_t* child_base, uint32_t* counts, hipStream_t stream);
// Set-mode branching: FirstSmallestVar by CARDINALITY (or InputOrder: the first variable of cardinality > 1), MiddleVal on the bounds, BinarySplit on the sets.
hipError_t launch_set_branch(uint32_t n_nodes, uint32_t n_vars, uint32_t set_words, int32_t base, uint32_t words, const uint64_t* bits, const int32_t* lb,
                             const int32_t* ub, const uint64_t* active, const uint8_t* status, uint64_t* child_bits, uint64_t* child_active,
                             uint32_t* child_base, uint32_t* counts, uint32_t reverse, uint32_t var_select, hipStream_t stream);

// Set-mode branching under Enumerate (pcp_branch_device_set_enum): the same variable, the member of its set nearest to MiddleVal's / MinVal's
// value, children x = v / x != v folded into the set.  counts[6] = error (3: an Unknown node without a variable of cardinality > 1).
hipError_t launch_set_branch_enum(uint32_t n_nodes, uint32_t n_vars, uint32_t set_words, int32_t base, uint32_t words, const uint64_t* bits, const int32_t* lb,
                                  const int32_t* ub, const uint64_t* active, const uint8_t* status, uint32_t val, uint64_t* child_bits, uint64_t* child_active,
                                  uint32_t* child_base, uint32_t* counts, uint32_t reverse, uint32_t var_select, hipStream_t stream);

// One step of the device-side DFS after the fixpoint of the top node: count it, branch it in place (right child over the parent's
// row, left child on top) or pop it, keep the first solution.
hipError_t launch_dfs_step(uint32_t n_vars, int32_t* lb, int32_t* ub, const uint8_t* status, uint32_t capacity, uint32_t* sp, uint32_t* stop,
                           unsigned long long* counters, int32_t* first_solution, uint32_t stop_on_solution, unsigned long long node_limit,
                           uint32_t* team_scratch, uint32_t team_words, uint32_t var_select, hipStream_t stream);

// On-device branching (FirstSmallestVar | InputOrder / MiddleVal / BinarySplit): scan of the Unknown flags, then one block per node.
hipError_t launch_branch(uint32_t n_nodes, uint32_t n_vars, uint32_t words, const int32_t* lb, const int32_t* ub, const uint64_t* active,
                         const uint8_t* status, int32_t* child_lb, int32_t* child_ub, uint64_t* child_active, uint32_t* child_dirty, uint32_t* child_base,
                         uint32_t* counts, uint32_t reverse, uint32_t var_select, hipStream_t stream);

// Enumerate on the device (pcp_enum.hip, pcp_branch_device_excl), behind launch_branch_scan: per Unknown node the variable, the value and the
// number of entries each child keeps (pick [n_nodes], cnt [2 n_nodes]: context scratch), the offsets of the child rows' lists, then the rows
// and the kept entries.  counts[5] = entries written, counts[6] = error (the children are then left unwritten).
hipError_t launch_enum_branch(uint32_t n_nodes, uint32_t n_vars, const int32_t* lb, const int32_t* ub, const uint32_t* child_base, const uint32_t* excl_off,
                              const pcp_excl* excl, uint32_t val, uint2* pick, uint32_t* cnt, int32_t* child_lb, int32_t* child_ub, uint32_t* child_dirty,
                              uint32_t* child_excl_off, pcp_excl* child_excl, uint32_t child_excl_capacity, uint32_t* counts, uint32_t reverse,
                              uint32_t var_select, hipStream_t stream);

// Branch and bound (pcp_bnb.hip, pcp_propagate_device_bnb): the incumbent folded into each node's objective domain before the fixpoint
// (empty[i] = 1: the fold would empty node i, its row is left as it was), then the empty nodes forced to PCP_FALSE and the best PCP_TRUE node
// of the batch taken as the new incumbent if it beats it.  Interval mode: lb / ub rows; set mode: bits rows (lb / ub ignored by the fold).
hipError_t launch_bnb_fold(uint32_t n_nodes, uint32_t n_vars, uint32_t var, uint32_t mode, const int32_t* best, int32_t* lb, int32_t* ub, uint64_t* bits,
                           uint32_t set_words, int32_t base, uint8_t* empty, hipStream_t stream);
hipError_t launch_bnb_reduce(uint32_t n_nodes, uint32_t n_vars, uint32_t var, uint32_t mode, const uint8_t* empty, uint8_t* status, const int32_t* lb_out,
                             const int32_t* ub_out, const uint64_t* bits_out, uint32_t set_words, int32_t* best, int32_t* best_lb, int32_t* best_ub,
                             uint64_t* best_bits, uint32_t* improved, hipStream_t stream);

// The variable selector's key for variable v of `size` > 1 values; the minimum over a node's variables is the choice, ~0 = none is open.
// FirstSmallestVar (first_smallest_var.rs:30-39) orders by (size, index); InputOrder (input_order.rs:30-39) by the index alone: the size
// is masked out of the key (option "var_select", wave-uniform: size_mask = var_size_mask(var_select), one 32-bit scalar — the key's upper
// half is the size's lower 32 bits, as `size << 32` always made it).
static __device__ __forceinline__ uint32_t var_size_mask(uint32_t var_select) { return var_select == PCP_VAR_INPUT_ORDER ? 0u : ~0u; }
static __device__ __forceinline__ unsigned long long var_key(unsigned long long size, uint32_t v, uint32_t size_mask) {
  return ((unsigned long long)((uint32_t)size & size_mask) << 32) | v;
}

}  // namespace pcp
