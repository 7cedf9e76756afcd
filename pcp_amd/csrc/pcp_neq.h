// pcp_neq.h — launch interfaces of the specialised fixpoint kernels (pcp_neq.hip: all-XNeqY models, assignment-driven;
// pcp_big.hip: binary models on 10-bit LDS cells), shared with the C-ABI host code.
#pragma once
#include "pcp_internal.h"

namespace pcp {

// The solution sink of a context (pcp_solution_sink_set) or of one call (pcp_dfs_forest_device_neq_sink): an append buffer of (lb, ub) rows
// every tree of an Interval forest writes its solutions into.  A solution draws a ticket from *count BEFORE it is counted; a ticket >= capacity hands the node back to the caller
// (error kDfsSinkFull, the contract of error 1).  The SINK = false instantiations never read the struct.
struct SinkDev {
  int32_t* lb;        // [capacity][n_vars]
  int32_t* ub;
  uint32_t* tree;     // [capacity] or null: the tree that wrote the row
  uint32_t* count;    // tickets drawn since the caller last zeroed it
  uint32_t capacity;
};
constexpr uint32_t kDfsSinkFull = 6;  // counters[t][3]: the sink was full — the node stays on the stack, propagated and uncounted

// Assignment-driven fixpoint of all-XNeqY models, implicit-active nodes (pcp_neq.hip): no sweep over the record table — round 0
// walks the adjacency lists of the variables that are singletons in the staged domains.
struct NeqArgs {
  ModelDev m;                   // needs adj_off, adjp, const_val, n_vars, n_slots (< 65536), n_recs, max_deg
  const uint32_t* adjp4;        // [adj_off[n_vars] + 1] (a zero entry behind the last list) 4-byte payloads (other | is_y << 15 | t << 16) when slots < 32768 and |offsets| < 32768, else null
  const uint32_t* seed_always;  // [ceil(n_slots/32)] bit v = variable v has a Constant neighbour (walked in round 0 whatever its domain), or null
  uint32_t n_nodes;
  uint32_t nodes_per_block;     // B <= 16 nodes per workgroup, domains in LDS node-major
  uint32_t packed;              // 1 = 16-bit (-lb, ub) cells (declared hull within +-kPackedMax), 0 = int2 cells
  uint32_t lds_wgs;             // workgroups meant to share a CU's LDS (sizes the jump-window area; must match lds_bytes_neq's argument)
  uint32_t* tile_ctr;           // or null: nine words 128 bytes apart, zero between launches — [32 r] the next ticket of residue r = blockIdx.x & 7 (tile = tile_static * gridDim.x + 8 * ticket + r), [256] workgroups that finished (the last one zeroes all nine)
  uint32_t tile_static;         // tiles a workgroup takes by the fixed stride before it draws tickets (>= 1)
  uint32_t stagger;             // option "neq_stagger": shader cycles by which the workgroup in a CU's second pair of wave slots delays its start (0 = none)
  uint32_t debug;               // profiling only ("neq_debug"; results are WRONG when non-zero): 1 = no rounds, 2 = no status scan, 4 = round 0 only
  uint32_t* violation;          // sticky device word: a node was refused with PCP_STATUS_HULL
  unsigned long long* dbg;      // [PCP_DBG_COUNT] diagnostic counters of the context (pcp_debug_counters); slots 5..15: phase timers under debug & 32
  unsigned long long* trace;    // profiling (option "neq_trace_ptr"): [grid][16 wavefronts][16 events] s_memtime stamps, or null
  const uint32_t* sp_ptr;       // host-stepped device-side DFS: the node to run is row *sp_ptr - 1 (see LaunchArgs)
  const uint32_t* stop_ptr;
  struct {                      // n_steps > 0: the search loop itself runs in ONE workgroup (grid 1, nodes_per_block 1): pcp_dfs_device
    uint32_t* sp;               //   lb_in/ub_in = lb_out/ub_out = the stack's rows [capacity][n_vars]; status [capacity]
    uint32_t* stop;
    unsigned long long* counters;  // nodes, solutions, failed nodes, error, internal (pcp_hip.h)
    int32_t* first_solution;
    uint32_t* dirty;            //   [capacity] per stack row: the variable it was branched on (>= n_vars: none), or null
    uint32_t capacity;
    uint32_t n_steps;
    uint32_t stop_on_solution;
    unsigned long long node_limit;
  } dfs;
  uint32_t cell_rows;           // 1 = pcp_device_batch.cell_format PCP_CELLS_PACKED16: lb_in / lb_out are rows of 32-bit cells (-lb & 0xffff | ub << 16), ub_* unused
  const uint32_t* dirty;        // pcp_device_batch.dirty_var: [n_nodes] the one variable in which node i differs from a fixpoint (>= n_vars: none), or null
  const int32_t* lb_in;
  const int32_t* ub_in;
  int32_t* lb_out;
  int32_t* ub_out;
  uint8_t* status;
  pcp_stats* stats;
  const uint32_t* excl_off;     // pcp_propagate_device_excl: [n_nodes + 1] CSR offsets into excl, or null (then the EXCL kernels are not launched)
  const pcp_excl* excl;         //   the nodes' own value exclusions x(var) != value (Enumerate's right branches), 8 bytes each
  struct {                      // dfs.n_steps > 0 and row_base != null: the search loop runs under Enumerate (pcp_dfs_forest_device_neq_enum, the DFS && EXCL kernels)
    pcp_excl* path;             //   [trees][path_capacity]: the exclusions along each tree's current path — the current node's list is path[t][0 .. n)
    uint32_t* row_base;         //   [trees][dfs.capacity]: the path entries a stack row inherits
    pcp_excl* row_excl;         //   [trees][dfs.capacity]: the entry appended when the row is popped (var 0xFFFFFFFF: none)
    uint32_t path_capacity;
    uint32_t val;               //   PCP_VAL_MIDDLE / PCP_VAL_MIN
  } en;
  SinkDev sink;                 // pcp_dfs_forest_device_neq_sink (the DFS && SINK kernels): the call's solution sink; sink.lb == null: none
                                // (the last member: the kernel arguments in front of it keep their offsets)
};
size_t lds_bytes_neq(uint32_t n_slots, uint32_t n_vars, uint32_t nodes_per_block, bool packed, uint32_t wgs = 2);
hipError_t launch_neqfix(const NeqArgs& a, const LaunchPlan& p, hipStream_t stream);
// int32 bounds rows <-> rows of packed cells (n = nodes x variables entries); a bound that does not fit sets *violation
hipError_t launch_pack_rows(const int32_t* lb, const int32_t* ub, uint32_t* cells, size_t n, uint32_t* violation, hipStream_t stream);
hipError_t launch_unpack_rows(const uint32_t* cells, int32_t* lb, int32_t* ub, size_t n, hipStream_t stream);
// the brancher over rows of cells; child_base from launch_branch_scan (pcp_kernels.hip), which also fills counts
hipError_t launch_branch_cells(uint32_t n_nodes, uint32_t n_vars, const uint32_t* cells, const uint32_t* child_base, uint32_t* child_cells, uint32_t* child_dirty,
                               const uint32_t* counts, uint32_t reverse, hipStream_t stream);

// Binary models whose store fits LDS only as 10-bit cells (declared hull of at most 1024 values), implicit-active nodes, one node
// per workgroup (pcp_big.hip).
// The records as that kernel reads them: 8 bytes with the CELL COORDINATES of both operands (slot s lives in word s / 3, field s % 3):
//   .x = word_x | field_x << 15 | (d & 0x1fff) << 17 | kind << 30        .y = word_y | field_y << 15
// and the adjacency payload of a variable's list entry (BigAdj), in the order of ModelDev::adj:
//   .x = word_other | field_other << 15 | (this variable is the record's y) << 17 | kind << 18        .y = d
struct BigArgs {
  ModelDev m;          // needs adj_off, const_val, n_recs, n_vars, n_slots (< 98304)
  const uint2* brec;   // [padded like ModelDev::recs] BigRec, sorted by kind (stable)
  const uint2* badj;   // [adj_off[n_vars]] BigAdj
  uint32_t dense_k;    // a wake-up round is dense iff dense_k * (list entries of the changed variables) >= records (option "big_dense_k")
  uint32_t has_unary;  // the model has records with a Constant operand (unary records, kind 3)
  uint32_t n_nodes;
  int32_t lo10;        // the hull's lower bound
  uint32_t round_mode; // option "big_round": 0 = every wake-up round takes the cheaper form, 1 = always dense, 2 = always sparse (tests)
  uint32_t* violation; // sticky device word: a node was refused with PCP_STATUS_HULL
  unsigned long long* dbg;  // [PCP_DBG_COUNT] diagnostic counters of the context (pcp_debug_counters)
  const uint32_t* sp_ptr;   // host-stepped device-side DFS: the node to run is row *sp_ptr - 1 (see LaunchArgs)
  const uint32_t* stop_ptr;
  const int32_t* lb_in;
  const int32_t* ub_in;
  int32_t* lb_out;
  int32_t* ub_out;
  uint8_t* status;
  pcp_stats* stats;
};
size_t lds_bytes_big(uint32_t n_vars, uint32_t n_slots);
hipError_t launch_bigfix(const BigArgs& a, const LaunchPlan& p, hipStream_t stream);

// Stores with formula propagators (the reified layer): every unit as a tree, one lane per unit (pcp_formula.hip).
using FNode = pcp_fnode;  // leaf: first = record index; inner node: first = index of its first child (children consecutive)
struct FormArgs {
  ModelDev m;                // needs recs, const_val, sums, n_vars, n_slots
  const FNode* nodes;        // the trees of all units
  const uint32_t* unit_root; // [n_units + 1] root node of each unit, then the number of nodes (a unit's nodes are unit_root[u] .. unit_root[u + 1])
  uint32_t n_units;
  uint32_t n_nodes;
  uint32_t* violation;
  const uint32_t* sp_ptr;    // host-stepped device-side DFS: the node to run is row *sp_ptr - 1 (see LaunchArgs)
  const uint32_t* stop_ptr;
  const int32_t* lb_in;
  const int32_t* ub_in;
  int32_t* lb_out;
  int32_t* ub_out;
  const uint64_t* active_in; // [n_nodes][ceil(n_units/64)] or null = every unit active
  uint64_t* active_out;      // or null
  uint8_t* status;
  pcp_stats* stats;
};
size_t lds_bytes_formula(uint32_t n_slots, uint32_t n_units, uint32_t waves);  // one slice per wavefront (= per node in flight)
hipError_t launch_formfix(const FormArgs& a, const LaunchPlan& p, hipStream_t stream);

// Such stores whose implicit nodes carry value exclusions of their own, optionally under branch and bound (pcp_formexcl.hip,
// pcp_propagate_device_form_excl): formfix_kernel's mapping; of `f`, active_in / sp_ptr / stop_ptr are not read.
struct FormExclArgs {
  FormArgs f;
  const uint32_t* excl_off;   // [n_nodes + 1] CSR offsets into excl (the first need not be 0), or null: no node has any
  const pcp_excl* excl;       //   x(var) != value, 8 bytes each
  uint32_t obj_var, obj_mode; // branch and bound (obj_best != null): the objective variable (< n_vars), PCP_MINIMIZE / PCP_MAXIMIZE
  const int32_t* obj_best;    //   device int32[1]: the incumbent, folded into the objective's cell as a node is staged; null = no objective
  uint8_t* empty;             //   [n_nodes]: receives 1 where the fold would empty the node (PCP_FALSE, row unchanged), else 0: bnb_reduce_kernel's input
};
hipError_t launch_formexcl(const FormExclArgs& a, const LaunchPlan& p, hipStream_t stream);

// What the two row-stack search forests of Interval stores share (row_dfs, pcp_rowdfs.hpp): one tree per WAVEFRONT on its own stack of
// (lb, ub) rows, a pcp_dfs_state laid out as for pcp_dfs_forest_device.  Embedded as `d` in FormDfsArgs and SmallDfsArgs, as SetDfsArgs is in
// SetFormDfsArgs.
struct RowDfsArgs {
  uint32_t n_trees, capacity, n_steps, stop_on_solution;
  unsigned long long node_limit; // per tree
  int32_t* lb;                   // [n_trees][capacity][n_vars]
  int32_t* ub;
  uint32_t* sp;                  // [n_trees]
  uint32_t* stop;                // [n_trees]
  unsigned long long* counters;  // [n_trees][5]: nodes, solutions, failed nodes, error, first-solution flag
  int32_t* first_solution;       // [n_trees][n_vars] or null
  uint32_t* violation;
  pcp_stats* stats;
  // branch and bound only (row_dfs<true, ..>: the _bnb entries, pcp_dfs_forest_device_small_enum / _form_enum with an objective)
  uint32_t obj_var, obj_mode;    // the objective variable, PCP_MINIMIZE / PCP_MAXIMIZE
  int32_t* obj_best;             // device int32[1]: the forest's incumbent
  int32_t* tree_best;            // [n_trees]: the value of each tree's last solution
  int32_t* tree_row;             // [n_trees][n_vars] or null: its lower bounds
  // Enumerate only (row_dfs<.., true, ..>, pcp_dfs_forest_device_small_enum / _form_enum; row_base == null: BinarySplit)
  pcp_excl* path;                // [n_trees][path_capacity]: the exclusions along each tree's current path
  uint32_t* row_base;            // [n_trees][capacity]: the path entries a stack row inherits
  pcp_excl* row_excl;            // [n_trees][capacity]: the entry appended when the row is popped (var 0xFFFFFFFF: none)
  uint32_t path_capacity, val;   // PCP_VAL_MIDDLE / PCP_VAL_MIN
  SinkDev sink;                  // the context's solution sink (row_dfs<false, .., true>); sink.lb == null: none
  uint32_t var_select;           // PCP_VAR_FIRST_SMALLEST / PCP_VAR_INPUT_ORDER (option "var_select"): read by the launchers, which choose the
                                 // instantiation by it (row_dfs<.., INPUT_ORDER>); the kernels do not read it.  The last member: the kernel
                                 // arguments in front of it keep their offsets
};

// The search loop over such a store on the device: the node being run in its tree's LDS slice (pcp_formdfs.hip).
struct FormDfsArgs {
  ModelDev m;                    // needs recs, const_val, sums, n_vars, n_slots
  const FNode* nodes;
  const uint32_t* unit_root;
  uint32_t n_units;
  RowDfsArgs d;
};
size_t lds_bytes_formdfs(uint32_t n_slots, uint32_t n_units, uint32_t waves);  // one slice per tree; 0 = beyond a CU's LDS
// (a.d.sink.lb != null: the instantiation that appends every solution to the sink; never together with bnb)
hipError_t launch_formdfs(const FormDfsArgs& a, bool bnb, const LaunchPlan& p, hipStream_t stream);

// The same stores over IntervalSet<i32> domains (set mode): the trees as above, the node's sets as bit words in LDS (pcp_setform.hip).
struct SetFormArgs {
  ModelDev m;                // needs recs, const_val, n_vars, n_slots
  const FNode* nodes;
  const uint32_t* unit_root;
  uint32_t n_units;
  uint32_t n_nodes;
  uint32_t set_words;        // u64 words per variable
  int32_t base;              // value v of a variable is bit v - base of its words (the hull's lower bound)
  const uint64_t* bits_in;   // [n_nodes][n_vars][set_words]
  uint64_t* bits_out;        // may be bits_in
  int32_t* lb_out;           // [n_nodes][n_vars] the bounds of the final sets
  int32_t* ub_out;
  const uint64_t* active_in; // [n_nodes][ceil(n_units/64)] or null = every unit active
  uint64_t* active_out;      // or null
  uint8_t* status;
  pcp_stats* stats;
};
size_t lds_bytes_setform(uint32_t n_vars, uint32_t set_words, uint32_t n_units, uint32_t waves);  // one slice per wavefront; 0 = beyond a CU's LDS
hipError_t launch_setformfix(const SetFormArgs& a, bool implicit, const LaunchPlan& p, hipStream_t stream);

// The search loop over such a store on the device: one tree per WAVEFRONT, the current node in its LDS slice, an undo trail in HBM
// (pcp_setformdfs.hip).  The forest's state, levels, trail and objective are setdfs_kernel's (SetDfsArgs `d`; of d.m: recs, const_val,
// n_recs, n_vars, n_slots), so setdfs_split_kernel serves this forest as it is.
struct SetFormDfsArgs {
  SetDfsArgs d;
  const FNode* nodes;
  const uint32_t* unit_root;
  uint32_t n_units;
};
size_t lds_bytes_setformdfs(uint32_t n_vars, uint32_t set_words, uint32_t n_units, uint32_t waves);  // one slice per tree; 0 = beyond a CU's LDS
// (sink.bits != null: the instantiation that appends every solution to the set sink, SetSinkDev of pcp_internal.h; never together with bnb)
hipError_t launch_setformdfs(const SetFormDfsArgs& a, const SetSinkDev& sink, bool enumerate, bool bnb, const LaunchPlan& p, hipStream_t stream);

// Small stores — a few dozen variables, up to a few thousand filters — over explicit `active` rows or implicit nodes: one wavefront per node
// (pcp_small.hip).
struct SmallArgs {
  ModelDev m;                 // needs recs, const_val, sums, n_recs, n_vars, n_slots
  const uint32_t* rec_unit;   // [n_recs] unit of each record, or null: every record is its own unit
  uint32_t n_units;
  uint32_t n_nodes;
  const uint32_t* ad_tab;     // all-different units, or null: [n, then (unit, count <= 64, first index into ad_vars) each]
  const uint32_t* ad_vars;    //   their variables
  const uint32_t* ad_mask;    //   bit u = unit u is one of them
  uint32_t* violation;
  unsigned long long* dbg;    // [kStatSlots][PCP_DBG_COUNT]
  const uint32_t* sp_ptr;     // host-stepped device-side DFS: the node to run is row *sp_ptr - 1 (see LaunchArgs)
  const uint32_t* stop_ptr;
  const uint32_t* nu_off;     // pcp_propagate_device_units: [n_nodes + 1] CSR offsets into nu, or null
  const pcp_prop* nu;         //   the nodes' own unary propagators (one variable against one Constant)
  const int32_t* lb_in;
  const int32_t* ub_in;
  int32_t* lb_out;
  int32_t* ub_out;
  const uint64_t* active_in;  // [n_nodes][ceil(n_units/64)] or null = every unit active
  uint64_t* active_out;       // or null
  uint8_t* status;
  pcp_stats* stats;
};
size_t lds_bytes_small(uint32_t n_slots, uint32_t n_units, uint32_t n_recs, uint32_t waves);
hipError_t launch_smallfix(const SmallArgs& a, const LaunchPlan& p, hipStream_t stream);

// Small stores whose implicit nodes carry value exclusions of their own, optionally under branch and bound (pcp_smallexcl.hip,
// pcp_propagate_device_small_excl): smallfix_kernel's mapping; of `s`, active_in / sp_ptr / stop_ptr / nu_off / nu are not read.
struct SmallExclArgs {
  SmallArgs s;
  const uint32_t* excl_off;   // [n_nodes + 1] CSR offsets into excl (the first need not be 0), or null: no node has any
  const pcp_excl* excl;       //   x(var) != value, 8 bytes each
  uint32_t obj_var, obj_mode; // branch and bound (obj_best != null): the objective variable (< n_vars), PCP_MINIMIZE / PCP_MAXIMIZE
  const int32_t* obj_best;    //   device int32[1]: the incumbent, folded into the objective's cell as a node is staged; null = no objective
  uint8_t* empty;             //   [n_nodes]: receives 1 where the fold would empty the node (PCP_FALSE, row unchanged), else 0: bnb_reduce_kernel's input
};
hipError_t launch_smallexcl(const SmallExclArgs& a, const LaunchPlan& p, hipStream_t stream);

// The search loop over such a store on the device (RowDfsArgs `d`): the node being run in its tree's LDS slice, the records in the copy its
// workgroup shares (pcp_smalldfs.hip).
struct SmallDfsArgs {
  ModelDev m;                    // needs recs, const_val, sums, n_recs, n_vars, n_slots
  const uint32_t* rec_unit;      // [n_recs] unit of each record, or null: every record is its own unit
  uint32_t n_units;
  const uint32_t* ad_tab;        // all-different units, or null (SmallArgs)
  const uint32_t* ad_vars;
  RowDfsArgs d;
};
size_t lds_bytes_smalldfs(uint32_t n_slots, uint32_t n_units, uint32_t n_recs, uint32_t waves);  // the records' copy + one slice per tree; 0 = beyond a CU's LDS
// (a.d.sink.lb != null: the instantiations that append every solution to the sink; never together with bnb)
hipError_t launch_smalldfs(const SmallDfsArgs& a, bool bnb, const LaunchPlan& p, hipStream_t stream);

}  // namespace pcp
