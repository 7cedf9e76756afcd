/* pcp_hip.h — C ABI of libpcp_hip.so, the MI355X (gfx950) propagation-fixpoint engine.
 *
 * Drop-in boundary.  The reference (ptal/pcp, libpcp 0.7.0, pure Rust) has no FFI;
 * the seam it offers is the trait
 *     kernel::Consistency<VStore>::consistency(&mut self, &mut VStore) -> SKleene
 *                                                    (src/libpcp/kernel/consistency.rs:17-19)
 * as implemented by propagation::store::Store       (src/libpcp/propagation/store.rs:240-258)
 * and required of any constraint store by IntCStore  (src/libpcp/concept.rs:120-138).
 * Every entry point below is what a Rust `GpuCStore: IntCStore<VStore>` would bind through
 * `extern "C"` (the binding stub is in INTEGRATION.md); each cites the reference item it replaces.
 *
 * Conventions: plain pointers and sizes; no exceptions or aborts cross the boundary; every call
 * returns PCP_OK (0) or a negative pcp_err.  Where the reference panics on a contract violation
 * (assert!), this library returns PCP_ERR_CONTRACT.  A pcp_ctx is used from one host thread at a
 * time; distinct contexts are independent.  There is NO CPU fallback: if no HIP device is present
 * pcp_ctx_create fails with PCP_ERR_NODEVICE.
 */
#ifndef PCP_HIP_H
#define PCP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCP_ABI_VERSION 8 /* (formula units over set-mode stores came without a new number: no symbol and no layout changed, calls that
                             were refused with PCP_ERR_UNSUPPORTED now work; so did the variable selector InputOrder, option "var_select":
                             no symbol and no layout changed, the default selects what every entry selected before) */

/* Operand encodings for pcp_prop.var[i]. */
#define PCP_CONST 0xFFFFFFFFu /* operand is a term::Constant (term/constant.rs:43-68); off[i] = its value   */
#define PCP_NOVAR 0xFFFFFFFEu /* operand slot unused (var[2] of the binary kinds)                          */
#define PCP_SUM 0xC0000000u   /* var[i] = PCP_SUM | t: the operand is the term::Sum view number t (term/sum.rs:56-92,
                                 registered with pcp_model_push_sum); off[i] adds a constant (Addition over the Sum, and
                                 the constants / Addition offsets of its members folded together)                    */

/* Interval bounds and offsets must stay inside [-PCP_BOUND_MAX, PCP_BOUND_MAX] so that no filter can
 * overflow i32 (the reference wraps in release and panics in debug; SURVEY.md §7 "i32 overflow"). */
#define PCP_BOUND_MAX 0x1FFFFFFF

typedef enum {
  PCP_OK = 0,
  PCP_ERR_ARG = -1,         /* null pointer, bad size, bad enum                                         */
  PCP_ERR_CONTRACT = -2,    /* a reference assert! would fire: empty initial domain (variable/store.rs:136),
                               var >= n_vars (variable/store.rs:176-179), same var twice in one propagator
                               (reactors/indexed_deps.rs:69-77), bound/offset out of PCP_BOUND_MAX        */
  PCP_ERR_HIP = -3,         /* a HIP runtime call failed; pcp_last_error() has the text                   */
  PCP_ERR_NOMEM = -4,
  PCP_ERR_UNSUPPORTED = -5, /* e.g. XEqYMulZ over set-mode domains, a set-mode store larger than one CU's LDS    */
  PCP_ERR_NODEVICE = -6     /* no HIP device: the engine never falls back to a CPU path                   */
} pcp_err;

/* Elementary propagator kinds.  X, Y, Z are views: Identity(var) (term/identity.rs:47-70),
 * Addition(var, off) (term/addition.rs:80-110) or Constant(off) (term/constant.rs:43-68). */
typedef enum {
  PCP_NEQ = 0,  /* XNeqY            propagators/cmp/x_neq_y.rs:66-104                                   */
  PCP_EQ = 1,   /* XEqY             propagators/cmp/x_eq_y.rs:67-116                                    */
  PCP_LT = 2,   /* XLessY           propagators/cmp/x_less_y.rs:67-117 (x>y, x>=y, x<=y are ctor sugar,
                                    propagators/cmp/mod.rs:34-60)                                        */
  PCP_LT3 = 3,  /* XLessYPlusZ      propagators/cmp/x_less_y_plus_z.rs:75-128                           */
  PCP_GT3 = 4,  /* XGreaterYPlusZ   propagators/cmp/x_greater_y_plus_z.rs:75-128                        */
  PCP_EQ3 = 5,  /* XEqYPlusZ = GT3(x+1,y,z) && LT3(x-1,y,z), one propagator
                                    propagators/cmp/x_eq_y_plus_z.rs:31-105                              */
  PCP_MUL3 = 6, /* XEqYMulZ         propagators/cmp/x_eq_y_mul_z.rs:68-115 (narrows x only)             */
  PCP_BOOL = 7, /* logic::Boolean   logic/boolean.rs:111-140: the formula "X = 1" over a 0/1 view (one operand)   */
  PCP_NBOOL = 8 /* logic::BooleanNeg logic/boolean_neg.rs:71-96: "X = 0"                                          */
} pcp_kind;

/* The reified layer (logic/): ONE unit = a tree of Conjunction (logic/conjunction.rs:77-119) and Disjunction
 * (logic/disjunction.rs:78-141) nodes over elementary leaves.  NotFormula::not is applied by the caller when the tree is built, as
 * the reference does (implication f g = Disjunction[f, g.not()], logic/mod.rs:30-36; equivalence = Conjunction of both
 * implications, logic/mod.rs:38-45): the engine only sees positive trees. */
typedef enum { PCP_F_LEAF = 0, PCP_F_AND = 1, PCP_F_OR = 2 } pcp_fnode_type;
typedef struct {
  uint8_t type;        /* pcp_fnode_type */
  uint8_t reserved;    /* must be 0 */
  uint16_t n_children; /* inner nodes: >= 1 */
  uint32_t first;      /* leaf: index into `leaves`; inner node: index in `nodes` of its first child (children are consecutive) */
} pcp_fnode;

/* SKleene as returned by Consistency::consistency (trilean::SKleene; propagation/store.rs:247-257). */
typedef enum { PCP_FALSE = 0, PCP_TRUE = 1, PCP_UNKNOWN = 2 } pcp_status;

/* One elementary filter.  A *unit* is what the reference stores as ONE Box<dyn PropagatorConcept>
 * (one index in Store::propagators, one bit of Store::active, propagation/store.rs:33-38):
 *   group_kind == 0 : the prop is a unit by itself;
 *   group_kind == 1 : consecutive props OF ONE pcp_model_push_props CALL carrying the same `group` value form ONE unit — a
 *                     logic::Conjunction (logic/conjunction.rs:77-119);
 *   group_kind == 2 : the same, built by Distinct::new (propagators/distinct.rs:63-83); it differs from
 *                     1 only in the ORDER of its reactor subscriptions (distinct.rs:117-124), which no
 *                     fixpoint depends on.  join_distinct (distinct.rs:26-45) instead pushes its pairs
 *                     as standalone units.
 * Units are numbered in push order; bit u of an `active` row is unit u. */
typedef struct {
  uint8_t kind;       /* pcp_kind */
  uint8_t group_kind; /* 0 standalone, 1 Conjunction member, 2 Distinct member */
  uint16_t reserved;  /* must be 0 */
  uint32_t group;     /* Conjunction id (only compared for equality with the previous prop) */
  uint32_t var[3];    /* variable index, PCP_CONST, or PCP_NOVAR */
  int32_t off[3];     /* Addition offset (0 = Identity) or the Constant's value */
} pcp_prop;

/* Counters.  A *filter step* = one evaluation of one elementary propagator's propagate()+is_subsumed()
 * (one scheduler pop, propagation/store.rs:166-175).  The reference keeps no such
 * counter.  Step counts are schedule-dependent: compare rates, never counts.
 * `steps`/`steps3` are REFERENCE-EQUIVALENT steps: every (propagator, node) pair the reference's scheduler would pop —
 * each live propagator once in the initial sweep (init_scheduler, store.rs:144-149) plus every wake-up.  The engine
 * proves most of the sweep's pairs no-ops in bulk (whole 64-propagator words from range tables of the tile's
 * domains) without looking at them; `evaluated` counts the pairs that WERE looked at one by one — tested on the
 * node's own domains (sweep level 1 / level 2, full filter) or run by a wake-up round — and `full_evals` the pairs
 * that ran the full filter (propagate() + is_subsumed() literally, with its domain writes). */
typedef struct {
  uint64_t steps;        /* reference-equivalent filter steps on binary kinds              */
  uint64_t steps3;       /* the same on ternary kinds (LT3/GT3/EQ3/MUL3)                   */
  uint64_t narrowings;   /* domain writes that strictly shrank a domain                    */
  uint64_t waves;        /* sum over nodes of fixpoint waves (>=1 per node)                */
  uint64_t failed_nodes; /* nodes that ended PCP_FALSE                                     */
  uint64_t nodes;        /* nodes propagated                                               */
  uint64_t evaluated;    /* (propagator, node) pairs tested individually on the node's domains */
  uint64_t full_evals;   /* pairs that ran the full filter                                 */
} pcp_stats;

typedef struct pcp_ctx pcp_ctx;

/* ---- context ------------------------------------------------------------------------------------ */
/* One context per CStore (the reference builds one Store per Space, search/space.rs:21-36). */
int32_t pcp_ctx_create(int32_t hip_device, pcp_ctx** out);
void pcp_ctx_destroy(pcp_ctx* ctx);
const char* pcp_last_error(const pcp_ctx* ctx); /* text of the last failing call on ctx (never NULL) */
const char* pcp_strerror(int32_t err);
uint32_t pcp_abi_version(void);

/* ---- model (≡ the immutable part of Store: `propagators`) ------------------------------------------ */
/* ≡ Store::empty() (propagation/store.rs:40-54) over a VStore of n_vars variables.
 *   set_words == 0 : Interval<i32> domains (VStoreFD, variable/mod.rs:36): bounds reasoning only.
 *   set_words  > 0 : IntervalSet<i32> domains (VStoreSet, variable/mod.rs:38 — the reference's default FDSpace,
 *                    search/mod.rs:41-43): every domain is a SET, carried as `set_words` u64 words per variable; value v is
 *                    bit (v - lo) where [lo, hi] is the hull declared with pcp_model_set_hull — REQUIRED in set mode, with
 *                    hi - lo < 64 * set_words.  XNeqY removes interior values, XEqY intersects sets, `active`/True follow
 *                    set disjointness.
 *   WHAT SET MODE REFUSES (PCP_ERR_UNSUPPORTED from pcp_model_push_props / _push_sum / _push_formula), and why:
 *     - XEqYMulZ over sets: the reference computes y.read() * z.read() with IntervalSet's Mul (x_eq_y_mul_z.rs:68-115), which lives in the
 *       third-party crate intervallum (not vendored in the reference tree, version pinned only by Cargo.lock); no test of the reference
 *       exercises it over IntervalSet, so neither the oracle nor this engine has anything to pin a set-valued product against.  The
 *       Interval<i32> product (bounds only) IS pinned (5 vectors, x_eq_y_mul_z.rs tests) and is what interval mode runs.
 *     - Sum views over sets (term/sum.rs:56-92): Sum::read adds IntervalSets member by member — the same unpinned third-party algebra
 *       (IntervalSet + IntervalSet); the reference's only Sum users (cumulative.rs) are tested over Interval stores.
 *     Both also apply to the leaves of a formula unit.  The reified layer itself (Boolean / BooleanNeg / formula units) RUNS over sets: the
 *     oracle's IntervalSet instantiation pins it, and a leaf's is_subsumed() is decided on the sets (XEqY is False iff they are disjoint).
 *     The search forest over sets has one entry per kind of store: pcp_dfs_forest_device_set, _set_enum and _set_bnb evaluate records, not
 *     formula trees, and return PCP_ERR_UNSUPPORTED for a store with formula propagators; pcp_dfs_forest_device_setform and _setform_bnb
 *     search exactly those stores and return it for a store without one.  pcp_dfs_forest_split_set serves both.
 *   THE SEARCH FORESTS, one row per kind of store:
 *     all-XNeqY, Interval            pcp_dfs_forest_device, pcp_dfs_forest_device_neq_enum, _neq_sink (any size the in-kernel search takes: N-queens-1000)
 *     formula units, Interval        pcp_dfs_forest_device_form, _form_bnb, _form_enum (what Cumulative::join builds: XEqYMulZ and Sum keep it here)
 *     records, IntervalSet           pcp_dfs_forest_device_set, _set_enum, _set_bnb
 *     formula units, IntervalSet     pcp_dfs_forest_device_setform, _setform_bnb
 *     small stores, Interval         pcp_dfs_forest_device_small, _small_bnb, _small_enum (plain propagators of any kind, <= 128 slots, <= 2048 filters: Golomb)
 *     any other Interval store has no forest: pcp_dfs_device searches it, one tree.
 *   ENUMERATE (search/branching/enumerate.rs:33-60: children `x = v` and `x != v`) needs no engine support in set mode — both children are
 *   exact set operations the caller applies to `bits` before propagating (keep bit v / clear bit v), as pcp_branch_device_set does for
 *   BinarySplit.  In interval mode `x != v` with v inside (lb, ub) is not a domain operation: it stays a per-node propagator — a unit
 *   pushed with pcp_model_push_props before the node's call and removed with pcp_model_truncate after it (what the host twins do for
 *   every branch constraint), or, for a BATCH of nodes with different such propagators each, pcp_propagate_device_units (ABI v8). */
int32_t pcp_model_reset(pcp_ctx* ctx, uint32_t n_vars, uint32_t set_words);
/* ≡ Store::alloc, append-only (propagation/store.rs:223-230). */
int32_t pcp_model_push_props(pcp_ctx* ctx, uint32_t n, const pcp_prop* props);
/* Registers a term::Sum view over n_members variables (term/sum.rs:30-32) and returns its number in *term; a prop refers to
 * it as var[i] = PCP_SUM | term.  read = the interval sum of the members (sum.rs:76-81); an update through a Sum of several
 * variables never narrows anything — it fails iff the new domain does not overlap the sum (sum.rs:66-69); a Sum of ONE
 * variable forwards to it (sum.rs:63-64).  The propagator depends on every member (sum.rs:85-91), so naming a variable twice
 * in one propagator — directly or through its Sums — is PCP_ERR_CONTRACT like the reference's reactor panic.  Interval mode
 * only.  pcp_model_reset forgets the terms. */
int32_t pcp_model_push_sum(pcp_ctx* ctx, uint32_t n_members, const uint32_t* vars, uint32_t* term);
/* ≡ Store::alloc of ONE formula propagator: nodes[0] is the root, at most 8 levels deep; leaves are elementary props (group fields
 * ignored; Sum operands allowed).  Its dependencies are the sorted, de-duplicated union of its leaves' (conjunction.rs:107-118,
 * disjunction.rs:119-131), so a variable may occur in several leaves.  A pop of the unit runs Disjunction::propagate literally: a
 * child is propagated only when every other child is disentailed.  Where the reference would PANIC — Boolean::propagate on a domain
 * without 1 reached through a Conjunction (a non-monotonic update, variable/store.rs:153-156) — the node fails instead.
 * Both domain types: over Interval stores the unit runs in pcp_formula.hip, over IntervalSet stores (set mode) in pcp_setform.hip, where
 * Boolean::propagate clears every other value of the set.  XEqYMulZ leaves and Sum operands stay interval mode only.
 * A tree of more than 64 nodes must be a flat Conjunction of leaves (the kernels keep a tree's statuses in 64-bit masks and walk a wider
 * unit as a loop over its members): this call takes any other one, and the first propagation or search call on the store — the lowering
 * runs there, before any launch — returns PCP_ERR_UNSUPPORTED until the unit is truncated away. */
int32_t pcp_model_push_formula(pcp_ctx* ctx, uint32_t n_nodes, const pcp_fnode* nodes, uint32_t n_leaves, const pcp_prop* leaves);
/* ≡ FrozenStore::restore's `propagators.truncate(label.0)` (propagation/store.rs:319-323); n_units counts
 * units, not elementary props. */
int32_t pcp_model_truncate(pcp_ctx* ctx, uint32_t n_units);
int32_t pcp_model_n_units(const pcp_ctx* ctx, uint32_t* n_units, uint32_t* n_props);
/* Optional: [lo, hi] = hull of the initial domains the variables were allocated with (VStore::alloc,
 * variable/store.rs:130-139).  Updates are monotone (variable/store.rs:156-170), so every domain of every node of the
 * search lies inside it.  With a hull within +-16383 the engine keeps the domains as 16-bit cells (twice the nodes per
 * workgroup) without the second, 32-bit launch it otherwise queues behind every such call for nodes that do not fit.
 * A node whose bounds leave the declared hull is a contract violation: pcp_propagate returns PCP_ERR_CONTRACT;
 * pcp_propagate_device leaves that node's outputs untouched, sets its status to PCP_STATUS_HULL and raises a sticky device
 * flag: the next pcp_stats_read returns PCP_ERR_CONTRACT however many launches happened in between (pcp_branch_device counts
 * such nodes in counts[4]).  pcp_model_reset forgets the hull.
 * The same refusal (status PCP_STATUS_HULL, outputs untouched, sticky flag) meets a node of pcp_propagate_device with a bound
 * beyond +-PCP_BOUND_MAX, hull or not: every tile checks the bounds it stages. */
int32_t pcp_model_set_hull(pcp_ctx* ctx, int32_t lo, int32_t hi);
#define PCP_STATUS_HULL 0xFE

/* ---- propagation (≡ Consistency::consistency, propagation/store.rs:247-257) ---------------------------- */
/* Host-buffer form: n_nodes independent spaces sharing the model.
 *   lb, ub  : [n_nodes][n_vars] i32, node-major, in/out (Interval<i32> bounds).  Set mode: OUT only (bounds of the sets).
 *   bits    : interval mode: must be NULL.  Set mode: [n_nodes][n_vars][set_words] u64 in/out, the domains.
 *   active  : [n_nodes][ceil(n_units/64)] u64 in/out; bit u == Store::active of unit u.  NULL = every unit
 *             active on entry, result not returned.
 *   status  : [n_nodes] out, pcp_status.
 *   stats   : nullable; counters of THIS call.
 * Post-condition: for status != PCP_FALSE, (lb,ub) are the reference's fixpoint domains and
 * `active` has lost exactly the entailed units; for PCP_FALSE nodes domains/active are unspecified. */
int32_t pcp_propagate(pcp_ctx* ctx, uint32_t n_nodes, int32_t* lb, int32_t* ub, uint64_t* bits,
                      uint64_t* active, uint8_t* status, pcp_stats* stats);

/* Device-resident form: all pointers are HIP device pointers on ctx's device; work is enqueued on
 * `hip_stream` (a hipStream_t, NULL = the null stream) and NOT synchronised.  *_out may alias *_in.
 * active_in NULL = all units active; active_out NULL = do not write the mask back.
 * IMPLICIT-ACTIVE NODES: with active_in == NULL a node is its domains only — no `active` rows are read or kept: a unit that
 * is entailed runs as a no-op, so liveness is derived (a unit is inactive iff it is entailed under the current domains,
 * SURVEY.md A.4); the status comes from an entailment scan of the final domains and active_out, when given, is
 * materialised from them.  Results are identical to passing all-ones rows; a search whose root has every unit active
 * (every driver) never needs rows at all (pcp_branch_device accepts active == child_active == NULL). */
typedef struct {
  const int32_t* lb_in;
  const int32_t* ub_in;
  int32_t* lb_out;
  int32_t* ub_out;
  const uint64_t* active_in;
  uint64_t* active_out;
  uint8_t* status;
  const uint64_t* bits_in; /* set mode only: [n_nodes][n_vars][set_words]; lb_in/ub_in are then ignored (may be NULL) */
  uint64_t* bits_out;      /* set mode only; may alias bits_in                                                        */
  /* ABI v7, optional (NULL = none): [n_nodes] — per node the ONE variable whose domain differs from a fixpoint of this same model, or
   * PCP_NOVAR (any value >= n_vars) = no promise, the node is propagated from scratch.  The caller PROMISES: take the node's row, give
   * that variable back the domain it had, and the row is the result of a consistency() over this model (a parent's fixpoint; a
   * child = the parent with one branch constraint folded in, which is what pcp_branch_device_hint writes).  Legal because a propagator
   * that is entailed or quiescent at a fixpoint is a no-op until one of ITS variables changes (propagation/store.rs:191-198 wakes exactly
   * the propagators of changed variables; the reference's prepare() re-schedules everything, store.rs:144-149, and finds the others
   * no-ops — DESIGN.md 2): the fixpoint, the status and the derived `active` rows are the same with and without the hint, only the
   * work differs.  Used by the all-XNeqY kernel (interval mode, implicit nodes); every other path ignores it.  A hint that breaks the
   * promise gives an unspecified (sound but possibly not fully propagated) result. */
  const uint32_t* dirty_var;
  /* ABI v7: the format of the bounds rows.  0 (PCP_CELLS_I32, the default): lb / ub are two int32 rows per node.  1 (PCP_CELLS_PACKED16): ONE
   * row of n_vars 32-bit CELLS per node, cell = (-lb & 0xffff) | ub << 16 — the format the all-XNeqY kernel keeps in LDS — in lb_in / lb_out;
   * ub_in / ub_out are ignored.  4 n_vars bytes per node instead of 8: staging is a copy, open-node stacks and records halve.  Needs a
   * declared hull within +-16383 (pcp_model_set_hull), an all-XNeqY model over implicit nodes (active_in == active_out == NULL), interval
   * mode; anything else: PCP_ERR_UNSUPPORTED.  pcp_pack_rows / pcp_unpack_rows convert on the device. */
  uint32_t cell_format;
  uint32_t reserved;
} pcp_device_batch;
#define PCP_CELLS_I32 0u
#define PCP_CELLS_PACKED16 1u
/* int32 rows <-> packed cells, [n_nodes][n_vars] each, device pointers, enqueued on hip_stream.  A bound outside +-16383 cannot be packed:
 * its cell is clamped and the context's sticky hull flag is raised (the next pcp_stats_read returns PCP_ERR_CONTRACT). */
int32_t pcp_pack_rows(pcp_ctx* ctx, uint32_t n_nodes, const int32_t* lb, const int32_t* ub, uint32_t* cells, void* hip_stream);
int32_t pcp_unpack_rows(pcp_ctx* ctx, uint32_t n_nodes, const uint32_t* cells, int32_t* lb, int32_t* ub, void* hip_stream);
/* pcp_branch_device_hint over rows of packed cells (implicit nodes): the same brancher, the same child order (option branch_reverse), the same
 * counts and hints; child_cells has room for 2 n_nodes rows.  A search whose open nodes stay cells between launches needs nothing else. */
/* (This brancher selects FirstSmallestVar only: under option var_select = PCP_VAR_INPUT_ORDER it returns PCP_ERR_UNSUPPORTED and launches
 * nothing; pcp_branch_device_hint on int32 rows honours the option.) */
int32_t pcp_branch_device_cells(pcp_ctx* ctx, uint32_t n_nodes, const uint32_t* cells, const uint8_t* status, uint32_t* child_cells,
                                uint32_t* child_dirty, uint32_t* counts, void* hip_stream);
int32_t pcp_propagate_device(pcp_ctx* ctx, uint32_t n_nodes, const pcp_device_batch* batch, void* hip_stream);
/* ABI v8 — nodes with propagators of their OWN.  In the reference every branch appends ONE unary propagator to ONE node's cstore
 * (Branch::distribute, search/branching/branch.rs:36-55); BinarySplit's  x <= v / x > v  and Enumerate's  x = v  narrow their variable once and are
 * then entailed, so a driver folds them into the child's bounds (what pcp_branch_device does) — but Enumerate's  x != v  with v INSIDE the
 * domain removes nothing on an Interval (x_neq_y.rs:82-93: only at a bound) and stays active until v reaches a bound
 * (search/branching/enumerate.rs:48-59).  Such propagators travel with their node:
 *   node_unit_off : device uint32 [n_nodes + 1], CSR offsets into node_units (NULL = no node has any: exactly pcp_propagate_device)
 *   node_units    : device pcp_prop [node_unit_off[n_nodes]] — kind PCP_NEQ / PCP_EQ / PCP_LT over ONE variable and ONE Constant in either
 *                   operand position (var[i] = PCP_CONST, off[i] = the value; the variable's off = its Addition offset); group fields ignored.
 * They are scheduled with the model's propagators (every one once, then again while anything narrows) and count in the node's status: a
 * node is PCP_TRUE only if its own propagators are entailed too.  Their liveness is not reported (`active` rows cover the model's units): a
 * caller drops a node unit when its constant has left the domain.  A malformed unit refuses its node (PCP_STATUS_HULL, sticky flag).
 * Interval mode, stores of at most 128 variables (interned constants included) and 2048 elementary filters — the one-wavefront-per-node
 * kernel (plan.path 4) —, int32 rows; anything else: PCP_ERR_UNSUPPORTED.  (Set mode needs none of this: there x != v is an exact set
 * operation on `bits`.) */
int32_t pcp_propagate_device_units(pcp_ctx* ctx, uint32_t n_nodes, const pcp_device_batch* batch, const uint32_t* node_unit_off,
                                   const pcp_prop* node_units, void* hip_stream);
/* Node EXCLUSIONS — the narrow companion of pcp_propagate_device_units, on the assignment-driven all-XNeqY kernel (plan.path 1): stores of
 * any size that fit LDS (N-queens-1000), packed cells, hints, the worklist rounds.  Of the unary propagators a branch appends only Enumerate's
 * right branch  x != v  over an Identity variable (search/branching/enumerate.rs:54-59) cannot be folded into bounds by the caller: on
 * Interval<i32> it removes a value only at a bound (x_neq_y.rs:82-93), so with v inside the domain it removes nothing and stays in that ONE
 * node's cstore until v reaches a bound.  An exclusion list is data that travels with a node, 8 bytes per entry — what a brancher writes:
 *   excl_off : device uint32 [n_nodes + 1], CSR offsets into excl (NULL = no node has any: exactly pcp_propagate_device)
 *   excl     : device pcp_excl [excl_off[n_nodes]]
 * Node i is propagated as if  XNeqY(Identity(var), Constant(value))  had been allocated behind the model's propagators once for each entry of
 * excl[excl_off[i] .. excl_off[i + 1])  — what Branch::distribute does (search/branching/branch.rs:36-55).  The exclusions are scheduled with
 * the model's propagators (every one once, then again while anything narrows) and count in the status: a node is PCP_TRUE only if every
 * exclusion is entailed too (its value lies outside [lb, ub]); x assigned to an excluded value gives PCP_FALSE.  Any number of exclusions per
 * node, duplicates and any order are allowed.  Their liveness is not reported: the caller drops an exclusion once its value has left the
 * domain.  An entry with var >= n_vars refuses that node only (PCP_STATUS_HULL, outputs untouched, sticky flag).
 * pcp_stats: every test of an exclusion is one step; a node's initial schedule (n_recs steps) grows by its number of exclusions.
 * Accepted: interval mode, an all-XNeqY model whose store fits LDS, implicit nodes (active_in == NULL; active_out on request), int32 rows,
 * dirty_var hints.  Anything else returns PCP_ERR_UNSUPPORTED with a message: set mode (it needs none of this), formula propagators, any other
 * model, a store that does not fit LDS, cell_format != 0, options force_path 2 / global_dom, the device DFS stack.
 * Enqueued on hip_stream, not synchronised, no host read-back. */
typedef struct {
  uint32_t var;   /* an Identity view, < n_vars */
  int32_t value;  /* x(var) != value */
} pcp_excl;
int32_t pcp_propagate_device_excl(pcp_ctx* ctx, uint32_t n_nodes, const pcp_device_batch* batch, const uint32_t* excl_off, const pcp_excl* excl,
                                  void* hip_stream);
/* Branch and bound — the reference's minimize / maximize (search/branch_and_bound.rs:64-84).  Once a solution is known, every node entered
 * gets one extra unary propagator before its propagation: Minimize  XLessY(var, Constant(best))  (var < best), Maximize  x_greater_y(var,
 * Constant(best))  (var > best).  It narrows its variable once and is then entailed, so it is folded into the node's domain, like
 * BinarySplit's branch constraints.  On a Satisfiable node the incumbent becomes  var.lower()  in BOTH modes.
 *   var       : the objective variable (an Identity view, < n_vars)
 *   mode      : PCP_MINIMIZE / PCP_MAXIMIZE
 *   best      : device int32[1], in/out: the incumbent.  "No solution yet" is PCP_BOUND_MAX + 1 (minimize) or -(PCP_BOUND_MAX + 1)
 *               (maximize): the fold is then a no-op.
 *   best_lb / best_ub : device [n_vars] or NULL: receive the lb_out / ub_out row of the node that set the incumbent
 *   best_bits : set mode, device [n_vars][set_words] or NULL: that node's sets
 *   improved  : device uint32[1] or NULL: +1 per call that improved the incumbent (accumulated, the caller zeroes it)
 * pcp_propagate_device_bnb has the contract of pcp_propagate_device, plus, enqueued on hip_stream with no host synchronisation:
 *   FOLD   before the fixpoint, the incumbent read on the device tightens each node's objective domain (interval mode: one bound; set mode:
 *          the objective's values >= best resp. <= best are cleared).  Rows in place (*_in == *_out) cost one column per node; otherwise the
 *          rows are copied to *_out first and propagated there.
 *   EMPTY  a node whose objective domain the fold empties is left as it was (a valid row: no hull check, no sticky flag) and comes out
 *          PCP_FALSE on every path.  pcp_stats counts the fixpoint launch as it ran.
 *   REDUCE after the fixpoint, the PCP_TRUE node with the best lb_out[var] (minimize: smallest, maximize: largest; a tie goes to the lowest
 *          node index) replaces the incumbent if it beats it: *best, the rows above and *improved are updated.
 * dirty_var is IGNORED: every node is propagated from scratch — the fold may narrow another variable than the hinted one, which breaks the
 * hint's promise.  cell_format PCP_CELLS_PACKED16: PCP_ERR_UNSUPPORTED.  var >= n_vars or an unknown mode: PCP_ERR_ARG. */
#define PCP_MINIMIZE 0u
#define PCP_MAXIMIZE 1u
typedef struct {
  uint32_t var;
  uint32_t mode;
  int32_t* best;
  int32_t* best_lb;
  int32_t* best_ub;
  uint64_t* best_bits;
  uint32_t* improved;
  uint32_t reserved;
} pcp_objective;
int32_t pcp_propagate_device_bnb(pcp_ctx* ctx, uint32_t n_nodes, const pcp_device_batch* batch, const pcp_objective* obj, void* hip_stream);
/* Node exclusions on SMALL stores of ANY plain model, optionally under branch and bound — Brancher<FirstSmallestVar, MiddleVal | MinVal, Enumerate>
 * (search/branching/enumerate.rs:33-60) over the stores pcp_propagate_device_units serves, on the lists pcp_branch_device_excl writes, with or
 * without BranchAndBound around it (search/branch_and_bound.rs:64-84).  (Added without a new ABI number: no layout changed.)
 *   excl_off, excl : as for pcp_propagate_device_excl — node i is propagated as if  XNeqY(Identity(var), Constant(value))  had been allocated behind
 *                    the model's propagators once for each entry of  excl[excl_off[i] .. excl_off[i + 1])  (search/branching/branch.rs:36-55): a value
 *                    is removed only at a bound, x assigned to it gives PCP_FALSE (x_neq_y.rs:82-93); an exclusion is entailed iff its value lies
 *                    outside [lb, ub] (x_neq_y.rs:71-73), and one that is not keeps the node PCP_UNKNOWN.  excl_off[0] need not be 0 (a slice of a
 *                    larger CSR); excl_off == NULL: no node has any.  Any number per node, duplicates and any order are allowed.  An entry with
 *                    var >= n_vars refuses that node only (PCP_STATUS_HULL, outputs untouched, sticky flag).  pcp_stats: every test of an entry is
 *                    one step.
 *   obj            : NULL: no branch and bound.  Otherwise the pcp_objective of pcp_propagate_device_bnb (best_bits unused), with its FOLD / EMPTY /
 *                    REDUCE contract, the fold done while each node is staged (no launch in front of the fixpoint): Minimize  ub = min(ub, best - 1),
 *                    Maximize  lb = max(lb, best + 1);  a node the fold would empty comes out PCP_FALSE with its *_out row equal to its *_in row,
 *                    in place or not.  var >= n_vars, an unknown mode, a null best, reserved != 0: PCP_ERR_ARG.
 * Accepted: interval mode, int32 rows, implicit nodes (active_in == NULL; active_out on request), a store without formula propagators of at most
 * 128 variables (interned constants included) and 2048 elementary filters that fits LDS — the one-wavefront-per-node kernel, plan.path 4; an
 * all-XNeqY model within those limits too.  dirty_var is ignored (every node is swept as a whole).  Anything else returns PCP_ERR_UNSUPPORTED
 * with a message: set mode, formula propagators, a larger store, cell_format != 0, active_in, the device DFS stack.
 * Enqueued on hip_stream, not synchronised, no host read-back. */
int32_t pcp_propagate_device_small_excl(pcp_ctx* ctx, uint32_t n_nodes, const pcp_device_batch* batch, const uint32_t* excl_off, const pcp_excl* excl,
                                        const pcp_objective* obj, void* hip_stream);
/* Node exclusions on stores WITH FORMULA UNITS, optionally under branch and bound — the same distributor over the stores pcp_model_push_formula
 * builds (schedules: propagators::Cumulative::join, cumulative.rs:59-114), which the two entries above refuse.  (Added without a new ABI number:
 * no layout changed.)
 *   excl_off, excl : as for pcp_propagate_device_small_excl, entry for entry: XNeqY(Identity(var), Constant(value)) behind the model's units; a value
 *                    is removed only at a bound, x assigned to it gives PCP_FALSE, an entry whose value lies inside [lb, ub] keeps the node
 *                    PCP_UNKNOWN even when every unit is entailed.  excl_off[0] need not be 0; excl_off == NULL: no node has any, and the call is
 *                    pcp_propagate_device on the same rows.  An entry with var >= n_vars refuses that node only (PCP_STATUS_HULL, outputs
 *                    untouched, sticky flag).  pcp_stats: every test of an entry is one step.
 *   obj            : as for pcp_propagate_device_small_excl (NULL: no branch and bound; the fold is done while each node is staged, a node the
 *                    fold would empty comes out PCP_FALSE with its *_out row equal to its *_in row).  var >= n_vars, an unknown mode, a null
 *                    best, reserved != 0: PCP_ERR_ARG.
 * Accepted: interval mode, int32 rows, implicit nodes (active_in == NULL; active_out on request), a store with formula propagators four nodes of
 * which fit one CU's LDS (8 bytes per variable and node) — formfix_kernel's one-wavefront-per-node mapping, plan.path 3.  Anything else returns
 * PCP_ERR_UNSUPPORTED with a message: set mode, a store without formula propagators (the two entries above serve those), cell_format != 0,
 * active_in, the device DFS stack.
 * Enqueued on hip_stream, not synchronised, no host read-back. */
int32_t pcp_propagate_device_form_excl(pcp_ctx* ctx, uint32_t n_nodes, const pcp_device_batch* batch, const uint32_t* excl_off, const pcp_excl* excl,
                                       const pcp_objective* obj, void* hip_stream);
/* One context = one queue of launches: the device-side scratch behind a launch (counters, team words, `active` scratch, the tile tickets of the
 * persistent kernels) belongs to the context, so the launches of one context must not overlap on the device — enqueue them on one stream, or order
 * the streams; concurrent launches take one context each (the model is uploaded per context).  The tile tickets are guarded at run time as well:
 * a ticketed launch enqueued on another stream than the context's last ticketed launch waits for that one (hipStreamWaitEvent), and after any HIP
 * error reported by this context the tickets are zeroed in front of the next launch that uses them. */

/* ---- branching on the device (the caller side of the path) -------------------------------------
 * ≡ Brancher<FirstSmallestVar, MiddleVal, BinarySplit>::enter (search/branching/brancher.rs:52-71) applied to every
 * PCP_UNKNOWN node of a propagated batch:
 *   variable = first index among the variables of minimal size > 1   (first_smallest_var.rs:30-39) or, under option var_select = PCP_VAR_INPUT_ORDER,
 *              the first index with size > 1   (input_order.rs:30-39)
 *   value    = (lb + ub) / 2 truncated toward zero                   (middle_val.rs:25-27)
 *   children = `x <= value` then `x > value`                          (binary_split.rs:46-57), folded into the bounds
 * (a var-vs-constant XLessY narrows its variable on its first run and is then entailed and unlinked, x_less_y.rs:87-109).
 * Children are written in tree order, two per Unknown node, each with a copy of its parent's `active` row — the
 * cstore label (len, active.clone()) of propagation/store.rs:315-317.  All pointers are device pointers.
 *   child_lb/child_ub : [2*n_nodes][n_vars] (capacity);  child_active : [2*n_nodes][ceil(n_units/64)]
 *   counts            : device uint32[5] out = { n_children, n_true, n_false, n_unknown, n_other } — n_other counts nodes whose
 *                       status is none of the three (PCP_STATUS_HULL: a node the engine refused); a driver should stop on it
 * Rows at or past n_children are not written.  A PCP_UNKNOWN node in which every variable is assigned has nothing to split (the
 * reference panics, first_smallest_var.rs:36; a propagated node is never one): its two children are plain copies of it, and
 * child_dirty holds 0xFFFFFFFF for both.
 * Nothing is synchronised; read `counts` after synchronising hip_stream. */
int32_t pcp_branch_device(pcp_ctx* ctx, uint32_t n_nodes, const int32_t* lb, const int32_t* ub, const uint64_t* active,
                          const uint8_t* status, int32_t* child_lb, int32_t* child_ub, uint64_t* child_active,
                          uint32_t* counts, void* hip_stream);
/* ABI v7: the same, and child_dirty [2*n_nodes] (capacity, nullable) receives for every child the variable it was branched on — the
 * pcp_device_batch.dirty_var entry of that child when its parent was a propagated (fixpoint) row, as it is in every search loop. */
int32_t pcp_branch_device_hint(pcp_ctx* ctx, uint32_t n_nodes, const int32_t* lb, const int32_t* ub, const uint64_t* active,
                               const uint8_t* status, int32_t* child_lb, int32_t* child_ub, uint64_t* child_active,
                               uint32_t* child_dirty, uint32_t* counts, void* hip_stream);

/* The same over FDSpace (set mode): FirstSmallestVar compares CARDINALITIES (first_smallest_var.rs:30-39: Domain::size()) — under option
 * var_select = PCP_VAR_INPUT_ORDER the variable is the first index with cardinality > 1 (input_order.rs:30-39) —, MiddleVal
 * is (lower + upper) / 2 of the set's bounds, the children keep the values <= value resp. > value of the variable's set.
 *   bits [n_nodes][n_vars][set_words], lb/ub [n_nodes][n_vars] = the outputs of pcp_propagate_device;
 *   child_bits [2*n_nodes][n_vars][set_words] (capacity); active / child_active as above (both NULL for implicit nodes). */
int32_t pcp_branch_device_set(pcp_ctx* ctx, uint32_t n_nodes, const uint64_t* bits, const int32_t* lb, const int32_t* ub, const uint64_t* active,
                              const uint8_t* status, uint64_t* child_bits, uint64_t* child_active, uint32_t* counts, void* hip_stream);

/* Enumerate over FDSpace (set mode):
 * ≡ Brancher<FirstSmallestVar, MiddleVal | MinVal, Enumerate>::enter (search/branching/brancher.rs:52-71, search/branching/enumerate.rs:47-60)
 * applied to every PCP_UNKNOWN node of a propagated set-mode batch.  On an IntervalSet XEqY(x, Constant v) intersects x with {v} and
 * XNeqY(x, Constant v) removes v wherever it sits, and both are then entailed: both children are folded into the variable's set, there are
 * no exclusion lists and the children are propagated like any other set-mode row.
 *   variable = first index among the variables of minimal CARDINALITY > 1   (first_smallest_var.rs:30-39 on Domain::size()) or, under option var_select = PCP_VAR_INPUT_ORDER,
 *              the first index with cardinality > 1   (input_order.rs:30-39)
 *   value    = PCP_VAL_MIN: m = lb of the variable (min_val.rs:25-27: lower(), always a member);  PCP_VAL_MIDDLE: m = (lb + ub) / 2 on a 64-bit
 *              sum, truncated toward zero (middle_val.rs:25-27).  The value is the member of the set nearest to m, m - d before m + d: m
 *              itself when it is a member — the reference; when it is not, the reference's left child fails, its right child is the parent
 *              again and the search does not end.
 *   children = `x = value` (the variable's set becomes {value}) then `x != value` (that bit is cleared); neither is ever empty.
 *   bits, lb, ub, active, child_bits, child_active : as for pcp_branch_device_set (active / child_active both NULL for implicit nodes)
 *   counts   : device uint32[8] out = { n_children, n_true, n_false, n_unknown, n_other, 0, error, 0 }, the first five as in
 *              pcp_branch_device.  error: 0 none; 3 an Unknown node without a variable of cardinality > 1 (the reference panics,
 *              first_smallest_var.rs:36).  On an error the children are unspecified and the inputs untouched.
 * Children come in tree order, two per Unknown node, x = value first; option branch_reverse reverses the rows as for pcp_branch_device.
 * Interval-mode model: PCP_ERR_UNSUPPORTED.  val > PCP_VAL_MIN or a null required pointer: PCP_ERR_ARG.  n_nodes == 0: PCP_OK, counts zeroed.
 * Everything is enqueued on hip_stream, nothing is synchronised.  (PCP_VAL_MIDDLE / PCP_VAL_MIN: below.) */
int32_t pcp_branch_device_set_enum(pcp_ctx* ctx, uint32_t n_nodes, const uint64_t* bits, const int32_t* lb, const int32_t* ub, const uint64_t* active,
                                   const uint8_t* status, uint32_t val, uint64_t* child_bits, uint64_t* child_active, uint32_t* counts,
                                   void* hip_stream);

/* The brancher that WRITES exclusion lists — the other half of pcp_propagate_device_excl:
 * ≡ Brancher<FirstSmallestVar, MiddleVal | MinVal, Enumerate>::enter (search/branching/brancher.rs:52-71, search/branching/enumerate.rs:47-60)
 * applied to every PCP_UNKNOWN node of a propagated batch whose node i carries the entries excl[excl_off[i] .. excl_off[i + 1]) (excl_off NULL =
 * no node has any; excl_off[0] need not be 0: a batch may be a slice of a larger CSR):
 *   variable = first index among the variables of minimal size > 1, sizes in 64 bits   (first_smallest_var.rs:30-39) or, under option var_select = PCP_VAR_INPUT_ORDER,
 *              the first index with size > 1   (input_order.rs:30-39)
 *   value    = PCP_VAL_MIDDLE: (lb + ub) / 2 truncated toward zero (middle_val.rs:25-27);  PCP_VAL_MIN: lb (min_val.rs:25-27).  A value the
 *              node has excluded already (an entry on the chosen variable) is not chosen again — on Interval<i32> an interior x != v removes
 *              nothing, so MiddleVal would choose it for ever —: the nearest value of [lb, ub] without an entry is taken, v - d before v + d.
 *   children = `x = value` then `x != value` (enumerate.rs:47-60).  x = value is folded into both bounds.  x != value is folded when the value
 *              is a bound of x (the lower bound: lb = value + 1; else the upper: ub = value - 1); otherwise the bounds stay and the entry
 *              (x, value) is appended BEHIND the inherited ones.  Each child inherits, in the parent's order, those of the parent's entries
 *              whose value lies inside [lb, ub] of their variable in that child's row (the others are entailed for good).  An entry with
 *              var >= n_vars is never used as an index: it is dropped from both children.
 *   child_lb / child_ub : [2*n_nodes][n_vars] (capacity);  child_dirty : [2*n_nodes] (capacity, nullable): the variable branched on
 *   child_excl_off      : [2*n_nodes + 1] (capacity): child_excl_off[0 .. n_children] is the CSR of the child ROWS, child_excl_off[0] = 0
 *   child_excl          : [child_excl_capacity].  n_child_excl <= 2 m + n_unknown, m = the number of entries of the Unknown nodes: a buffer of
 *                         that size always suffices.
 *   counts              : device uint32[8] out = { n_children, n_true, n_false, n_unknown, n_other, n_child_excl, error, 0 }, the first five
 *                         as in pcp_branch_device.  error: 0 none; 1 n_child_excl > child_excl_capacity; 3 an Unknown node without a variable
 *                         of size > 1 (the reference panics, first_smallest_var.rs:36); 4 every value of the chosen variable is excluded.
 *                         Several errors in one batch: the largest code.  On an error the first six counts are still valid (a node with
 *                         error 3 or 4 counts no entries), the children are unspecified and the inputs untouched: the call can be repeated.
 * Children come in tree order, two per Unknown node, x = value first; option branch_reverse reverses the rows (and with them the CSR) as for
 * pcp_branch_device.  The child buffers must not overlap the inputs.  Rows need no alignment and n_vars need not be a multiple of 4.
 * Accepted: interval mode, int32 rows, implicit nodes — the contract of pcp_propagate_device_excl, except that the model may be any.  Set mode:
 * PCP_ERR_UNSUPPORTED.  val > PCP_VAL_MIN or a null required pointer: PCP_ERR_ARG.  n_nodes == 0: PCP_OK, counts zeroed.
 * All pointers are device pointers; everything is enqueued on hip_stream, nothing is synchronised, nothing is allocated in steady state. */
#define PCP_VAL_MIDDLE 0u
#define PCP_VAL_MIN 1u
/* The variable selector, option "var_select" of the context (pcp_set_option), read by each entry when it is called:
 *   PCP_VAR_FIRST_SMALLEST (the default): the first index among the variables of minimal size > 1   (first_smallest_var.rs:30-39)
 *   PCP_VAR_INPUT_ORDER                 : the first index with size > 1                             (input_order.rs:30-39)
 * (set mode: cardinality for size).  Value choice, children, the exclusion rule, child_dirty and the errors are the same under both; error 3 —
 * an Unknown node with nothing to branch on — is the same case (the reference panics in both, input_order.rs:37).
 * WHERE "variable = first index among the variables of minimal size > 1" BECOMES "or, under PCP_VAR_INPUT_ORDER, the first index with size > 1":
 *   pcp_branch_device, _hint, _excl, _set, _set_enum;  pcp_dfs_device (on an all-XNeqY model it then takes its stepping path, as under
 *   "neq_dfs" 0);  pcp_dfs_forest_device_set, _set_enum, _set_bnb, _setform, _setform_bnb;  pcp_dfs_forest_device_form, _form_bnb,
 *   _form_enum, _small, _small_bnb, _small_enum, with and without a solution sink.  pcp_dfs_forest_split_set depends on levels, not on the
 *   selector.
 * WHERE IT DOES NOT RUN: under PCP_VAR_INPUT_ORDER pcp_dfs_forest_device and pcp_dfs_forest_device_neq_enum (the all-XNeqY in-kernel forest) and
 *   pcp_branch_device_cells (the packed-cell brancher) return PCP_ERR_UNSUPPORTED with a message naming the option and launch nothing. */
#define PCP_VAR_FIRST_SMALLEST 0u
#define PCP_VAR_INPUT_ORDER 1u
int32_t pcp_branch_device_excl(pcp_ctx* ctx, uint32_t n_nodes, const int32_t* lb, const int32_t* ub, const uint8_t* status,
                               const uint32_t* excl_off, const pcp_excl* excl, uint32_t val, int32_t* child_lb, int32_t* child_ub,
                               uint32_t* child_dirty, uint32_t* child_excl_off, pcp_excl* child_excl, uint32_t child_excl_capacity,
                               uint32_t* counts, void* hip_stream);

/* ---- the reference's search loop, one node per step, without the host in the loop -----------------------------------------------
 * ≡ OneSolution / AllSolution<Propagation<Brancher<FirstSmallestVar, MiddleVal, BinarySplit>>> over a VectorStack
 * (search/mod.rs:45-52, search/engine/one_solution.rs:92-105), optionally under StopNode (search/stop_node.rs:47-62): each step
 * pops the node on top of a LIFO stack of implicit-active nodes, runs its propagation fixpoint (one node = the reference's
 * one-consistency-call-per-node pattern, all CUs on that node), and branches it in place — exactly the reference's left-first
 * order.  n_steps steps are ENQUEUED on hip_stream with no host synchronisation in between: the kernels read the stack pointer
 * from device memory.  Steps after the stack has emptied (or `stop` was raised: solution found / node limit / error) do nothing.
 *   lb, ub           : [capacity][n_vars] device rows; rows [0, *sp) are the open nodes, row *sp - 1 the top
 *   sp, stop         : device uint32 each (the caller initialises *sp = 1 with the root in row 0, *stop = 0)
 *   status           : [capacity] device scratch
 *   counters         : device uint64[5] = { nodes, solutions, failed nodes, error (1 stack overflow: the node stays on the stack, uncounted;
 *                      2 hull violation; 3 an Unknown node without a variable to branch on — the reference panics, first_smallest_var.rs:36), internal },
 *                      accumulated (the caller zeroes them)
 *   first_solution   : [n_vars] device or NULL: the first solution found
 *   node_limit       : != 0 = StopNode(limit) nested as the reference nests it, Monitor<Statistics, StopNode<..>> (stop_node.rs:90-97): the node that
 *                      brings `nodes` to the limit is counted as a node and NEITHER as a solution nor as a failure (its status reaches the monitor as
 *                      EndOfSearch, stop_node.rs:57-62), and `stop` is raised.  The same rule in pcp_dfs_forest_device (per tree) and
 *                      pcp_dfs_forest_device_set (on total_nodes).
 * Interval mode only. */
typedef struct {
  int32_t* lb;
  int32_t* ub;
  uint32_t capacity;
  uint32_t* sp;
  uint32_t* stop;
  uint8_t* status;
  uint64_t* counters;
  int32_t* first_solution;
  /* ABI v7, nullable: [capacity] uint32 (pcp_dfs_forest_device: [n_trees][capacity]), one word per stack row = the variable that row was
   * branched on (the pcp_device_batch.dirty_var of the open node in that row), or >= n_vars for a row the caller put there (a root): the
   * engine writes it when it pushes children and, when it pops a row, propagates from that variable alone instead of from every assigned
   * variable of the node.  A caller that moves rows between stacks moves their words along.  All-XNeqY in-kernel loop only. */
  uint32_t* dirty;
} pcp_dfs_state;
/* (Variable: the first index among the variables of minimal size > 1 or, under option var_select = PCP_VAR_INPUT_ORDER, the first index with
 * size > 1 — input_order.rs:30-39; set mode: cardinality.  On an all-XNeqY model the option sends pcp_dfs_device down its stepping path, as "neq_dfs" 0 does) */
int32_t pcp_dfs_device(pcp_ctx* ctx, const pcp_dfs_state* st, uint32_t n_steps, uint32_t stop_on_solution, uint64_t node_limit, void* hip_stream);
/* The same loop on n_trees independent stacks at once, one workgroup per tree (ABI v5): tree t is exactly a pcp_dfs_device instance on
 *   lb, ub [n_trees][capacity][n_vars] (tree t's rows start at t * capacity), sp / stop [n_trees], status [n_trees][capacity],
 *   counters [n_trees][5], first_solution [n_trees][n_vars] or NULL;  node_limit applies to each tree.
 * The trees are the subtrees below the open nodes of a frontier (pcp_propagate_device + pcp_branch_device produce one); the caller adds
 * up the counters and decides when to stop launching (all sp == 0, any stop != 0, its node budget).  All-XNeqY models over implicit
 * nodes only (PCP_ERR_UNSUPPORTED otherwise: pcp_dfs_device runs any interval model, one tree). */
/* (Variable: the first index among the variables of minimal size > 1 or, under option var_select = PCP_VAR_INPUT_ORDER, the first index with
 * size > 1 — input_order.rs:30-39; set mode: cardinality.  THIS entry selects FirstSmallestVar only: under PCP_VAR_INPUT_ORDER it returns PCP_ERR_UNSUPPORTED and
 * launches nothing; pcp_dfs_forest_device_small takes an all-XNeqY store within its limits) */
int32_t pcp_dfs_forest_device(pcp_ctx* ctx, const pcp_dfs_state* st, uint32_t n_trees, uint32_t n_steps, uint32_t stop_on_solution, uint64_t node_limit, void* hip_stream);
/* The same forest for an Interval store WITH formula propagators (Boolean / BooleanNeg / pcp_model_push_formula units) — the stores
 * propagators::Cumulative::join builds (propagators/cumulative.rs:59-114: equivalences over Boolean, XEqYMulZ and Sum views, which set mode
 * refuses).  ≡ the engine of pcp_dfs_device (search/mod.rs:45-52, search/engine/one_solution.rs:92-105, under StopNode,
 * search/stop_node.rs:47-62) on n_trees stacks at once: tree t is exactly a pcp_dfs_device instance on slice t of the state, laid out as for
 * pcp_dfs_forest_device; `dirty` is ignored and may be NULL, `status` is scratch.  These stores are small, so a tree is one WAVEFRONT with
 * the node it runs in a slice of a CU's LDS, up to four trees per 256-thread workgroup: pcp_last_plan reports path 3, block = 64 x trees per
 * workgroup, grid = ceil(n_trees / those), lds_bytes.  Between two calls sp, the rows [0, sp), the counters and stop are what pcp_dfs_device
 * leaves after the same number of steps, node for node, so a caller may move bottom rows between stacks.  Unit liveness is derived, never
 * stored: the descent to a left child keeps it, every other pop sets every unit live.
 * Set-mode model, a null required buffer, n_trees == 0, capacity < 2: PCP_ERR_ARG.  A store without formula propagators:
 * PCP_ERR_UNSUPPORTED (all-XNeqY: pcp_dfs_forest_device; any other: pcp_dfs_device, one tree).  A node that does not fit one CU's LDS:
 * PCP_ERR_UNSUPPORTED.  n_steps == 0: PCP_OK, nothing is launched. */
/* (Variable: the first index among the variables of minimal size > 1 or, under option var_select = PCP_VAR_INPUT_ORDER, the first index with
 * size > 1 — input_order.rs:30-39; set mode: cardinality.) */
int32_t pcp_dfs_forest_device_form(pcp_ctx* ctx, const pcp_dfs_state* st, uint32_t n_trees, uint32_t n_steps, uint32_t stop_on_solution,
                                   uint64_t node_limit, void* hip_stream);

/* ---- the same loop over FDSpace (set mode), a FOREST of trees, one per workgroup (ABI v5) --------------------------------------
 * ≡ the engine above over VStoreSet = VStoreTrail<IntervalSet<i32>> (variable/mod.rs:38): like the reference, a node is restored
 * by undoing a TRAIL (variable/memory/trail_memory.rs:100-104) instead of being copied — a tree's current node stays in one CU's
 * LDS, every narrowing appends (word, removed bits) to the tree's trail, a backtrack ORs them back down to the level's mark and
 * takes the right branch.  Within a tree: exactly the reference's left-first order (FirstSmallestVar on CARDINALITIES, MiddleVal,
 * BinarySplit).  Several trees = the subtrees below the open nodes of a frontier (pcp_propagate_device + pcp_branch_device_set
 * produce one), searched concurrently; n_trees = 1 with the root in bits[0] IS the reference's search.  One call runs at most
 * n_steps nodes per tree; the caller repeats it until every tree is finished, `stop` is raised, or the budget is spent.
 *   bits        : [n_trees][n_vars][set_words] device: in = each tree's root, afterwards each tree's current node
 *   tree        : [n_trees][4] device uint32 = { levels, trail length, pending variable, finished | given << 8 }; the caller initialises every
 *                 tree to { 0, 0, PCP_DFS_FULL, 0 } (PCP_DFS_FULL: the current node has not been propagated at all)
 *   levels      : [n_trees][level_capacity][4] device uint32: the branch decisions whose right child is still open
 *   trail       : [n_trees][trail_capacity][4] device uint32
 *   counters    : [n_trees][4] device uint64 = { nodes, solutions, failed nodes, error (1 level stack full — the node stays current,
 *                 uncounted; 3 an Unknown node without a variable to branch on; 4 trail full: the tree cannot be restored; 5 internal round cap) }, accumulated
 *   total_nodes : device uint64: nodes of all trees; with node_limit != 0 no node beyond it is run (StopNode, stop_node.rs:57-62)
 *   stop        : device uint32: raised on a solution (stop_on_solution), at the node limit, on an error; the caller zeroes it
 *   first_solution / solution_flag : [n_vars] device int32 and a device uint32 (zeroed by the caller), or both NULL: the first solution
 *                 any tree reports (with several trees "first" is in time, not in the reference's order)
 * Set mode, implicit nodes. */
#define PCP_DFS_FULL 0xFFFFFFFFu
typedef struct {
  uint32_t n_trees, level_capacity, trail_capacity, reserved;
  uint64_t* bits;
  uint32_t* tree;
  uint32_t* levels;
  uint32_t* trail;
  uint64_t* counters;
  uint64_t* total_nodes;
  uint32_t* stop;
  int32_t* first_solution;
  uint32_t* solution_flag;
} pcp_forest_state;
/* (Variable: the first index among the variables of minimal size > 1 or, under option var_select = PCP_VAR_INPUT_ORDER, the first index with
 * size > 1 — input_order.rs:30-39; set mode: cardinality.) */
int32_t pcp_dfs_forest_device_set(pcp_ctx* ctx, const pcp_forest_state* st, uint32_t n_steps, uint32_t stop_on_solution, uint64_t node_limit, void* hip_stream);
/* The same loop under Brancher<FirstSmallestVar, MiddleVal | MinVal, Enumerate> (enumerate.rs:47-60): a level is `x = value, then x != value`
 * instead of `x <= value, then x > value`; variable and value as pcp_branch_device_set_enum chooses them (val: PCP_VAL_MIDDLE / PCP_VAL_MIN;
 * anything else: PCP_ERR_ARG), both children folded into the set through the trail.  State, counters, StopNode, first solution and errors
 * are those of pcp_dfs_forest_device_set; a level records its distributor (levels[..][3]: bit 0 = given away, bit 1 = Enumerate), so
 * pcp_dfs_forest_split_set hands over the right branch of either.  Roots expanded with pcp_branch_device_set_enum under the same val make
 * the union one Enumerate tree. */
/* (Variable: the first index among the variables of minimal size > 1 or, under option var_select = PCP_VAR_INPUT_ORDER, the first index with
 * size > 1 — input_order.rs:30-39; set mode: cardinality.) */
int32_t pcp_dfs_forest_device_set_enum(pcp_ctx* ctx, const pcp_forest_state* st, uint32_t val, uint32_t n_steps, uint32_t stop_on_solution,
                                       uint64_t node_limit, void* hip_stream);
/* Branch and bound around that loop — BranchAndBound<Propagation<Brancher<..>>> over FDSpace (search/branch_and_bound.rs:64-84; its test,
 * branch_and_bound.rs:112-138, runs this composition), under either distributor (enumerate 0: BinarySplit on MiddleVal; 1: Enumerate on val,
 * PCP_VAL_MIDDLE / PCP_VAL_MIN).  The forest shares ONE incumbent, the device word *best.  A tree entering a node — a root, a child, a right
 * branch, the node a launch resumes, a node received through pcp_dfs_forest_split_set — first clears from the objective's set the values
 * >= *best (minimize) or <= *best (maximize), read at that moment: the bound propagator of pcp_propagate_device_bnb, folded.  The removal
 * goes through the trail, so a backtrack undoes it and the right child folds again; a node whose objective the fold empties is a node and a
 * failed node.  On a solution the tree records var.lower() and the node's lower bounds as ITS latest — within a tree each beats the one
 * before — and then lowers / raises *best atomically.  Nothing is copied per node: the bound costs one device load and, when it narrows,
 * one trail entry per word.
 *   var, mode : the objective variable (< n_vars), PCP_MINIMIZE / PCP_MAXIMIZE
 *   best      : device int32[1], in/out: the incumbent; "no solution yet" as for pcp_objective: the fold is then a no-op.  A caller that
 *               seeds it with a known bound gets only solutions that beat it.
 *   tree_best : device [n_trees], the caller initialises every entry to that "no solution yet" value: the value of each tree's latest solution
 *   tree_row  : device [n_trees][n_vars] or NULL: the lower bounds of that solution.  Afterwards the optimum's row is tree_row[t] of any tree
 *               with tree_best[t] == *best (none: no solution beat the seeded incumbent).
 * State, counters, errors, StopNode (node_limit) and pcp_dfs_forest_split_set between calls are those of pcp_dfs_forest_device_set; there is no
 * stop on a solution — branch and bound runs to the end — and st->first_solution / st->solution_flag are ignored.  With n_trees = 1 the nodes
 * are the reference's, one for one; with several trees the optimum is the same and the node count depends on when each tree saw which incumbent.
 * Interval-mode model, var >= n_vars, mode > PCP_MAXIMIZE, enumerate > 1, val > PCP_VAL_MIN, a null best / tree_best: PCP_ERR_ARG. */
typedef struct {
  uint32_t var, mode;
  int32_t* best;
  int32_t* tree_best;
  int32_t* tree_row;
} pcp_forest_objective;
/* (Variable: the first index among the variables of minimal size > 1 or, under option var_select = PCP_VAR_INPUT_ORDER, the first index with
 * size > 1 — input_order.rs:30-39; set mode: cardinality.) */
int32_t pcp_dfs_forest_device_set_bnb(pcp_ctx* ctx, const pcp_forest_state* st, const pcp_forest_objective* obj, uint32_t enumerate, uint32_t val,
                                      uint32_t n_steps, uint64_t node_limit, void* hip_stream);
/* The same forest for a store WITH formula propagators (Boolean / BooleanNeg / pcp_model_push_formula units): the loop above under either
 * distributor (enumerate 0: BinarySplit on MiddleVal; 1: Enumerate on val, PCP_VAL_MIDDLE / PCP_VAL_MIN), every unit evaluated as a tree as
 * pcp_propagate_device does for such a store.  These stores are small, so a tree is one WAVEFRONT with its node in a slice of a CU's LDS, up to
 * four trees per 256-thread workgroup: pcp_last_plan reports block = 64 x trees per workgroup, grid = ceil(n_trees / those), lds_bytes, path 3.
 * State, counters, errors, StopNode, first solution, levels and trail are those of pcp_dfs_forest_device_set, byte for byte, and
 * pcp_dfs_forest_split_set hands work between the trees.  Unit liveness is derived, never stored: a descent keeps it, a backtrack and the
 * start of a call set every unit live.  With n_trees = 1 the nodes are the reference's, one for one.
 * Interval-mode model, enumerate > 1, val > PCP_VAL_MIN: PCP_ERR_ARG.  A store without formula propagators: PCP_ERR_UNSUPPORTED (it is
 * searched by pcp_dfs_forest_device_set).  A node that does not fit one CU's LDS: PCP_ERR_UNSUPPORTED. */
/* (Variable: the first index among the variables of minimal size > 1 or, under option var_select = PCP_VAR_INPUT_ORDER, the first index with
 * size > 1 — input_order.rs:30-39; set mode: cardinality.) */
int32_t pcp_dfs_forest_device_setform(pcp_ctx* ctx, const pcp_forest_state* st, uint32_t enumerate, uint32_t val, uint32_t n_steps,
                                      uint32_t stop_on_solution, uint64_t node_limit, void* hip_stream);
/* Branch and bound around it: pcp_dfs_forest_device_set_bnb for stores with formula propagators — the same objective struct, the same fold
 * of *best on entering a node, no stop on a solution.  Also PCP_ERR_ARG: var >= n_vars, mode > PCP_MAXIMIZE, a null best / tree_best. */
/* (Variable: the first index among the variables of minimal size > 1 or, under option var_select = PCP_VAR_INPUT_ORDER, the first index with
 * size > 1 — input_order.rs:30-39; set mode: cardinality.) */
int32_t pcp_dfs_forest_device_setform_bnb(pcp_ctx* ctx, const pcp_forest_state* st, const pcp_forest_objective* obj, uint32_t enumerate,
                                          uint32_t val, uint32_t n_steps, uint64_t node_limit, void* hip_stream);
/* Branch and bound around pcp_dfs_forest_device_form, the forest over Interval stores with formula propagators (above) —
 * BranchAndBound<Propagation<Brancher<..>>> (search/branch_and_bound.rs:64-84) — with the objective struct of the set forests.  The forest shares ONE incumbent, the device word *best.  Every row a tree pops first gets the bound
 * folded into the objective's domain, *best read at that moment: ub[var] = min(ub[var], best - 1) (minimize) or lb[var] = max(lb[var],
 * best + 1) (maximize); "no solution yet" as for pcp_objective: the fold is then a no-op.  A node the fold empties is a node and a failed
 * node.  The fold is written back with the node, so the right child inherits it and folds again when it is popped.  On a solution
 * tree_best[t] = lb[var], tree_row[t] = the node's lower bounds, then *best is lowered / raised atomically.  There is no stop on a solution,
 * and st->first_solution is ignored.  With n_trees = 1 the nodes are the reference's, one for one.
 * Also PCP_ERR_ARG: var >= n_vars, mode > PCP_MAXIMIZE, a null best / tree_best. */
/* (Variable: the first index among the variables of minimal size > 1 or, under option var_select = PCP_VAR_INPUT_ORDER, the first index with
 * size > 1 — input_order.rs:30-39; set mode: cardinality.) */
int32_t pcp_dfs_forest_device_form_bnb(pcp_ctx* ctx, const pcp_dfs_state* st, uint32_t n_trees, const pcp_forest_objective* obj,
                                       uint32_t n_steps, uint64_t node_limit, void* hip_stream);
/* The same forest for a SMALL Interval store of plain propagators — no formula units, at most 128 slots (variables and interned constants)
 * and 2048 elementary filters: Distinct, XLessY, XEqY, XEqYPlusZ, XLessYPlusZ, XGreaterYPlusZ, XEqYMulZ and Sum views in any mixture, the
 * stores the one-wavefront-per-node fixpoint kernel propagates (plan.path 4; the Golomb-ruler network is one).  State, counters, error
 * codes, StopNode and first solutions are those of pcp_dfs_forest_device_form: tree t is exactly a pcp_dfs_device instance on slice t of
 * the state, `dirty` is ignored and may be NULL, `status` is scratch, unit liveness is derived.  A tree is one WAVEFRONT, up to four trees
 * per 256-thread workgroup, which share one LDS copy of the records: pcp_last_plan reports path 4, block = 64 x trees per workgroup,
 * grid = ceil(n_trees / those), lds_bytes.  Option "small_alldiff" is honoured (0: a Distinct runs pair by pair — the same tree).  An
 * all-XNeqY store within the limits is accepted too.
 * Set-mode model, a null required buffer, n_trees == 0, capacity < 2: PCP_ERR_ARG.  A store with formula propagators: PCP_ERR_UNSUPPORTED
 * (pcp_dfs_forest_device_form).  A store over the limits, or whose records and one node do not fit one CU's LDS: PCP_ERR_UNSUPPORTED
 * (pcp_dfs_device searches it, one tree).  n_steps == 0: PCP_OK, nothing is launched. */
/* (Variable: the first index among the variables of minimal size > 1 or, under option var_select = PCP_VAR_INPUT_ORDER, the first index with
 * size > 1 — input_order.rs:30-39; set mode: cardinality.) */
int32_t pcp_dfs_forest_device_small(pcp_ctx* ctx, const pcp_dfs_state* st, uint32_t n_trees, uint32_t n_steps, uint32_t stop_on_solution,
                                    uint64_t node_limit, void* hip_stream);
/* Branch and bound around it, exactly as pcp_dfs_forest_device_form_bnb is around pcp_dfs_forest_device_form: one incumbent word *best for
 * the forest, folded into every popped row; tree_best / tree_row on a solution, then *best lowered / raised atomically; no stop on a
 * solution.  Also PCP_ERR_ARG: var >= n_vars, mode > PCP_MAXIMIZE, a null best / tree_best. */
/* (Variable: the first index among the variables of minimal size > 1 or, under option var_select = PCP_VAR_INPUT_ORDER, the first index with
 * size > 1 — input_order.rs:30-39; set mode: cardinality.) */
int32_t pcp_dfs_forest_device_small_bnb(pcp_ctx* ctx, const pcp_dfs_state* st, uint32_t n_trees, const pcp_forest_objective* obj,
                                        uint32_t n_steps, uint64_t node_limit, void* hip_stream);
/* The same forest under Brancher<FirstSmallestVar, MiddleVal | MinVal, Enumerate> (search/branching/enumerate.rs:33-60), with (obj != NULL)
 * or without branch and bound: a node's children are `x = v` and `x != v`, variable and value as pcp_branch_device_excl chooses them — v is
 * MiddleVal's or MinVal's value, or, when the node's list already holds (x, v), the nearest value of [lb, ub] without an entry on x, the
 * lower one first.  `x != v` with v at a bound is folded into that bound; an interior one stays with its node as a pcp_excl entry and is
 * propagated with the store at the top of every round as pcp_propagate_device_small_excl does (a value is removed only at a bound; x
 * assigned to it fails the node; an entry whose value lies inside [lb, ub] keeps the node PCP_UNKNOWN; every test of an entry is a step).
 * A depth-first tree needs no list per open node: every open row is the right child of an ancestor of the current node, so its list is a
 * prefix of the entries appended along the current path plus at most one entry of its own.
 *   path          : [n_trees][path_capacity] device pcp_excl: the exclusions along each tree's current path; may be NULL when path_capacity == 0
 *   row_base      : [n_trees][capacity] device uint32: how many path entries stack row r inherits
 *   row_excl      : [n_trees][capacity] device pcp_excl: the one entry appended behind them when row r is popped; var == 0xFFFFFFFF: none
 *   path_capacity : entries per tree
 *   val           : PCP_VAL_MIDDLE / PCP_VAL_MIN
 * THE STATE BETWEEN CALLS: for every row r in [0, sp) of tree t, node r is the row's bounds under the list path[t][0 .. row_base[t][r])
 * plus row_excl[t][r].  row_base does not decrease with r, and no length word is stored: a call derives the current list from the top row.  A
 * caller that moves a tree's bottom row to another tree moves its two words and the first row_base[0] path entries along (the donor's path
 * stays: its other rows use that prefix); a root is row 0 with its list in path[t][0 .. k), row_base = k and row_excl = none.  Entries are
 * never filtered out of the path: one whose value lies outside [lb, ub] is entailed for good.
 * Counters, StopNode, first solutions, stop_on_solution (ignored when obj != NULL), tree_best / tree_row and the errors are those of
 * pcp_dfs_forest_device_small / _small_bnb, and two more cases: error 5, "exclusion path full" — a popped row has an entry and
 * row_base == path_capacity: nothing is changed, the row stays on the stack, uncounted, stop is raised, and a caller that resumes with a
 * larger path runs it then (the contract of error 1); error 2 also for a path or row entry with var >= n_vars (never used as an index) or
 * a row_base beyond path_capacity: the node is counted and popped, the tree stops and the sticky violation flag is set.  With n_trees = 1
 * the nodes are search.dfs_enumerate's, one for one.  pcp_last_plan: as for pcp_dfs_forest_device_small (path 4).
 * Accepted stores: those of pcp_dfs_forest_device_small.  Set-mode model, val > PCP_VAL_MIN, a null required buffer (ex, row_base, row_excl,
 * path with path_capacity > 0), n_trees == 0, capacity < 2, a bad objective as for _small_bnb: PCP_ERR_ARG.  Formula propagators or a
 * store over the limits: PCP_ERR_UNSUPPORTED.  n_steps == 0: PCP_OK, nothing is launched. */
typedef struct {
  pcp_excl* path;
  uint32_t* row_base;
  pcp_excl* row_excl;
  uint32_t path_capacity;
  uint32_t val;
} pcp_forest_excl;
/* (Variable: the first index among the variables of minimal size > 1 or, under option var_select = PCP_VAR_INPUT_ORDER, the first index with
 * size > 1 — input_order.rs:30-39; set mode: cardinality.) */
int32_t pcp_dfs_forest_device_small_enum(pcp_ctx* ctx, const pcp_dfs_state* st, uint32_t n_trees, const pcp_forest_excl* ex,
                                         const pcp_forest_objective* obj, uint32_t n_steps, uint32_t stop_on_solution, uint64_t node_limit,
                                         void* hip_stream);
/* Enumerate in the forest of pcp_dfs_forest_device_form — Interval stores WITH formula propagators: schedules, what Cumulative::join builds —
 * with (obj != NULL) or without branch and bound: the signature and the contract of pcp_dfs_forest_device_small_enum over the stores of
 * pcp_dfs_forest_device_form.  `ex`, the state between calls, the counters, StopNode, first solutions, stop_on_solution (ignored when
 * obj != NULL), tree_best / tree_row and the errors 1, 2, 3, 5 and 6 are those of pcp_dfs_forest_device_small_enum.  A node's rounds are
 * those of pcp_propagate_device_form_excl: its exclusions at the top of every round, then every live unit.  With n_trees = 1 the nodes are
 * search.dfs_enumerate's over a store with formula units, one for one.  pcp_last_plan: as for pcp_dfs_forest_device_form (path 3).
 * Set-mode model, val > PCP_VAL_MIN, a null required buffer (st, ex, row_base, row_excl, path with path_capacity > 0), n_trees == 0,
 * capacity < 2, a bad objective as for _form_bnb: PCP_ERR_ARG.  A store WITHOUT formula propagators (pcp_dfs_forest_device_small_enum
 * searches it), a node that does not fit one CU's LDS, obj != NULL with a sink attached: PCP_ERR_UNSUPPORTED.  n_steps == 0: PCP_OK,
 * nothing is launched. */
/* (Variable: the first index among the variables of minimal size > 1 or, under option var_select = PCP_VAR_INPUT_ORDER, the first index with
 * size > 1 — input_order.rs:30-39; set mode: cardinality.) */
int32_t pcp_dfs_forest_device_form_enum(pcp_ctx* ctx, const pcp_dfs_state* st, uint32_t n_trees, const pcp_forest_excl* ex,
                                        const pcp_forest_objective* obj, uint32_t n_steps, uint32_t stop_on_solution, uint64_t node_limit,
                                        void* hip_stream);
/* Enumerate in the all-XNeqY forest of pcp_dfs_forest_device — Brancher<FirstSmallestVar, MiddleVal | MinVal, Enumerate>
 * (search/branching/enumerate.rs:33-60, search/branching/brancher.rs:52-71) inside the assignment-driven kernel, one WORKGROUP per tree: the
 * parameter list of pcp_dfs_forest_device_small_enum, for stores of any size pcp_dfs_forest_device accepts (N-queens-1000).
 * STORES: those of pcp_dfs_forest_device — all-XNeqY, interval mode, implicit nodes, a variable store that fits the in-kernel search.
 * TREES: tree t is slice t of `st`, laid out as for pcp_dfs_forest_device, `dirty` included (nullable; honoured under option "neq_hint").
 * EXCLUSION STATE: `ex` exactly as pcp_dfs_forest_device_small_enum documents it — path[t][path_capacity], row_base[t][capacity],
 *   row_excl[t][capacity], val in {PCP_VAL_MIDDLE, PCP_VAL_MIN}.  Node r of tree t is the row's bounds under path[t][0 .. row_base[t][r]) plus
 *   row_excl[t][r]; row_base does not decrease with r; a root is row 0 with its list in path[t][0 .. k), row_base = k and no entry; entries are
 *   never filtered out of the path.  A caller that moves a tree's bottom row to another tree moves its two words, its `dirty` word and the
 *   first row_base[0] path entries along (the donor's path stays).
 * NODE ORDER: the children are x = v, then x != v; the variable is FirstSmallestVar's; v is MiddleVal's or MinVal's value, or, when the node's
 *   list already holds (x, v), the nearest value of [lb, ub] without an entry on x, m - k tried before m + k.  x != v at a bound is folded into
 *   that bound; an interior one becomes the row's row_excl and joins the path when the row is popped.  With n_trees = 1 the nodes are those of
 *   search.dfs_enumerate at batch 1, one for one, and between two calls sp, the rows [0, sp), row_base, row_excl, the path prefix of the top
 *   row, the counters and stop are what pcp_dfs_forest_device_small_enum leaves after the same number of steps.  Both children carry
 *   dirty = x: also an interior right child, which differs from its parent's fixpoint by one entry that narrows nothing.
 * NODE STATUS: the node's entries are swept at the top of every round of its fixpoint (a value is removed only at a bound); an entry whose
 *   value lies inside [lb, ub] keeps the node PCP_UNKNOWN; x assigned to an excluded value fails the node.
 * Counters, StopNode (the limit node is a node, neither a solution nor a failure), first_solution and stop_on_solution are those of
 * pcp_dfs_forest_device.  pcp_last_plan: as for pcp_dfs_forest_device (path 1, grid = n_trees).
 * ERRORS (counters[t][3]): 1 — stack full: the node stays on the stack, propagated and uncounted (its row_base names its list, no entry);
 *   3 — as in pcp_dfs_forest_device; 5 — a popped row has an entry and row_base == path_capacity: nothing is changed, the row stays on the
 *   stack uncounted, stop is raised, and a caller that resumes with a larger path runs it then; 2 — a node the engine refused, also a path or
 *   row entry with var >= n_vars or a row_base beyond path_capacity (never used as an index): the node is counted and popped, the tree stops
 *   and the sticky violation flag is set.
 * REFUSALS (nothing is launched; pcp_last_error names the reason).  PCP_ERR_ARG: a set-mode model; val > PCP_VAL_MIN; a null st, ex, row_base
 *   or row_excl, a null stack buffer; a null path with path_capacity > 0; n_trees == 0; capacity < 2.  PCP_ERR_UNSUPPORTED: a store that is
 *   not all-XNeqY (formula units: pcp_dfs_forest_device_form_enum; any other small store: pcp_dfs_forest_device_small_enum); explicit-active
 *   nodes (option "implicit_active" 0); obj != NULL — there is no branch and bound in this forest (pcp_dfs_forest_device_small_enum); an
 *   Interval solution sink attached; option var_select = PCP_VAR_INPUT_ORDER (both as pcp_dfs_forest_device refuses them).
 *   n_steps == 0: PCP_OK, nothing is launched. */
int32_t pcp_dfs_forest_device_neq_enum(pcp_ctx* ctx, const pcp_dfs_state* st, uint32_t n_trees, const pcp_forest_excl* ex,
                                       const pcp_forest_objective* obj, uint32_t n_steps, uint32_t stop_on_solution, uint64_t node_limit,
                                       void* hip_stream);
/* The solution sink: every solution of an Interval forest, not only their number.  A device-side append buffer of (lb, ub) rows that every
 * tree of pcp_dfs_forest_device_form, pcp_dfs_forest_device_small, pcp_dfs_forest_device_small_enum and pcp_dfs_forest_device_form_enum
 * (the last two with obj == NULL) writes its solutions into — the visitor of AllSolution (search/engine/all_solution.rs), resp. OneSolution called in a loop (one_solution.rs:92-105).  A row is
 * the WHOLE node: in interval mode a True node is a box — every unit is entailed while domains may still be wider than one value — and
 * every point of it is a solution; first_solution keeps its lower bounds only.
 *   lb, ub   : [capacity][n_vars] device int32: row i = the i-th solution appended
 *   tree     : [capacity] device uint32 or NULL: the tree that wrote row i
 *   count    : device uint32: tickets drawn since the caller last zeroed it.  It may exceed capacity: the valid rows are min(*count, capacity)
 *   capacity : rows (> 0);  reserved : 0
 * The sink belongs to the context, like the options: the struct is copied at the call, the buffers stay the caller's, NULL detaches.  One
 * context is one queue of launches; the caller reads and zeroes *count between launches, never during one.
 * THE PROTOCOL.  A node found to be a solution (not the StopNode limit node, which is none: stop_node.rs:57-62) draws a ticket,
 * slot = (*count)++, BEFORE it is counted.  slot < capacity: the node's (lb, ub) go to row slot, tree[slot] = t, and the step goes on as
 * without a sink — the node is counted, first_solution kept, stop raised under stop_on_solution.  slot >= capacity: error 6, "sink full" —
 * nothing is counted, the node stays on the stack as row sp - 1, propagated (under Enumerate its row_base / row_excl name the list it ran
 * under, with no entry of its own), and stop is raised: the contract of error 1.  A caller that copies the rows out, zeroes *count, clears
 * that tree's error and stop and calls again runs the node again — propagation is idempotent — and it is counted and appended then.  So
 * after any number of such hand-backs nodes / solutions / failed of every tree are what a sink that never fills leaves, and no solution is
 * lost or written twice.  Rows are in ticket order, which between trees is an order in time.
 * With a sink attached the branch-and-bound entries (pcp_dfs_forest_device_form_bnb, _small_bnb, _small_enum and _form_enum with obj != NULL: they keep
 * tree_row), the all-XNeqY entries pcp_dfs_forest_device / pcp_dfs_forest_device_neq_enum — that forest writes its solutions through
 * pcp_dfs_forest_device_neq_sink, below, which takes its sink as an argument and refuses an attached one like them — and every set-mode forest
 * entry (pcp_dfs_forest_device_set, _set_enum, _set_bnb,
 * _setform, _setform_bnb) return PCP_ERR_UNSUPPORTED and launch nothing; with none attached every entry does what it did before.  (THIS
 * sink, of (lb, ub) rows, is meant: the set-mode forests write into a sink of their own, pcp_set_solution_sink below.)
 * A null lb, ub or count, capacity == 0, reserved != 0: PCP_ERR_ARG, and the sink attached before stays. */
typedef struct {
  int32_t* lb;
  int32_t* ub;
  uint32_t* tree;
  uint32_t* count;
  uint32_t capacity;
  uint32_t reserved;
} pcp_solution_sink;
int32_t pcp_solution_sink_set(pcp_ctx* ctx, const pcp_solution_sink* sink);
/* Every solution of the all-XNeqY forest — the visitor of AllSolution (search/engine/all_solution.rs) inside the assignment-driven kernel,
 * one WORKGROUP per tree.  The sink is an ARGUMENT OF THE CALL: the struct is read at the call and nothing is retained, the context's own
 * attachment (pcp_solution_sink_set) keeps its meaning, and this entry refuses it as pcp_dfs_forest_device and
 * pcp_dfs_forest_device_neq_enum do — one rule for every all-XNeqY entry.
 * ex == NULL: BinarySplit — stores, trees, node order, counters, StopNode, first_solution, stop_on_solution and errors 1, 2, 3 are those of
 *   pcp_dfs_forest_device.  ex != NULL: Enumerate — all of that, the exclusion state and error 5 are those of
 *   pcp_dfs_forest_device_neq_enum (with obj == NULL: there is no branch and bound in this forest).
 * THE PROTOCOL is pcp_solution_sink's, above.  A True node (not the StopNode limit node, which is none and draws no ticket:
 *   stop_node.rs:57-62) draws slot = (*count)++ BEFORE it is counted.  slot < capacity: the WHOLE node goes to row slot — in interval mode a
 *   True node of an all-XNeqY store is a box (x in [0,1], y in [3,4], x != y is entailed at the root), every point of it a solution —,
 *   tree[slot] = t, and the step goes on as without a sink.  slot >= capacity: error 6 in counters[t][3] — nothing is counted, the node stays
 *   on the stack as row sp - 1 at its fixpoint (under Enumerate its row_base names the list it ran under, row_excl no entry, as for errors 1
 *   and 3), stop[t] is raised.  A caller that copies the rows out, zeroes *count, clears that tree's error and stop and calls again runs the
 *   node again — propagating a fixpoint changes nothing, its `dirty` word is still valid — and it is counted and appended then.  After any
 *   number of such hand-backs nodes / solutions / failed of every tree are those of pcp_dfs_forest_device resp. _neq_enum on the same roots,
 *   and no solution is lost or written twice.  The valid rows are min(*count, capacity), in ticket order; rows beyond them are not touched.
 * REFUSALS (nothing is launched; pcp_last_error names the reason).  PCP_ERR_ARG: a null sink, lb, ub or count, capacity == 0,
 *   reserved != 0; a null st or stack buffer, n_trees == 0, capacity < 2; a set-mode model; with ex: val > PCP_VAL_MIN, a null row_base or
 *   row_excl, a null path with path_capacity > 0.  PCP_ERR_UNSUPPORTED: an Interval solution sink attached to the context; option
 *   var_select = PCP_VAR_INPUT_ORDER; explicit-active nodes (option "implicit_active" 0); a store that is not all-XNeqY (their forests write
 *   into the context's sink) or does not fit the in-kernel search.  n_steps == 0: PCP_OK, nothing is launched.
 * (Added without a new PCP_ABI_VERSION: a symbol more, no layout changed, every call that ran before runs as it did.) */
int32_t pcp_dfs_forest_device_neq_sink(pcp_ctx* ctx, const pcp_dfs_state* st, uint32_t n_trees, const pcp_forest_excl* ex,
                                       const pcp_solution_sink* sink, uint32_t n_steps, uint32_t stop_on_solution, uint64_t node_limit,
                                       void* hip_stream);
/* Between two calls of any Interval forest entry — pcp_dfs_forest_device, _form, _small, their _bnb and _enum forms, _neq_enum and _neq_sink:
 * idle trees take work from trees that have some, on the device.  What pcp_dfs_forest_split_set is to the set-mode forests; here the state
 * is a stack of rows, and the work handed over is the donor's BOTTOM row — its oldest open node, the subtree nearest its root.
 *   st, n_trees : the forest's state as its entries take it; rows are the context's n_vars wide.  Only lb, ub, sp, capacity and dirty
 *                 (nullable) are used.
 *   ex          : the exclusion state of the Enumerate forests, or NULL for the BinarySplit ones; `val` is ignored.
 *   pairs       : n_pairs x (donor, receiver) tree indices, device uint32
 *   done        : [n_pairs] device uint32: done[i] = 1 if pair i was carried out, else 0 and nothing belonging to that pair changes
 * A pair is VALID when donor != receiver, both are < n_trees, sp[receiver] == 0, 2 <= sp[donor] <= capacity and, with ex,
 * row_base[donor][0] <= path_capacity.  Validity is decided on the state as it was when the call was enqueued: a valid pair earlier in the
 * array does not change the verdict on a later one.  A tree may appear in at most ONE valid pair and in any number of invalid ones; no
 * index taken from an invalid pair is ever used to address memory.
 * A VALID PAIR (d, r), with k = sp[d] before the call:
 *   - row 0 of d — lb, ub and, when st->dirty is there, its dirty word — becomes row 0 of r;
 *   - with ex: the first nb = row_base[d][0] entries of d's path are copied to r's path, row_base[r][0] = nb, row_excl[r][0] = row_excl[d][0];
 *     d's path stays as it is (its other rows use that prefix);
 *   - rows 1 .. k-1 of d move down to 0 .. k-2, in lb, ub, dirty, row_base and row_excl;
 *   - sp[d] = k - 1, sp[r] = 1.
 * Counters, stop, status, first_solution and the per-tree branch-and-bound words are untouched, so the sum over the trees stays the
 * search's.  Nothing is specified for rows at or above a tree's new sp, or for entries of r's path at or beyond nb.  Trees in no valid pair
 * are untouched, bit for bit.
 * The entry does not look at the store kind: it works on the state alone.  Enqueued on hip_stream, not synchronised, no host read-back.
 * A set-mode model (pcp_dfs_forest_split_set serves those), a null st, lb, ub or sp, null pairs or done with n_pairs > 0, n_trees == 0,
 * capacity < 2, with ex a null row_base or row_excl or a null path with path_capacity > 0: PCP_ERR_ARG.  n_pairs == 0: PCP_OK, nothing is
 * launched.
 * (Added without a new PCP_ABI_VERSION: a symbol more, no layout changed, every call that ran before runs as it did.) */
int32_t pcp_dfs_forest_steal(pcp_ctx* ctx, const pcp_dfs_state* st, uint32_t n_trees, const pcp_forest_excl* ex /* NULL: BinarySplit forests */,
                             uint32_t n_pairs, const uint32_t* pairs, uint32_t* done, void* hip_stream);
/* TWO SINKS.  pcp_solution_sink, above, is the Interval forests': rows of (lb, ub).  While it is attached every set-mode forest entry
 * returns PCP_ERR_UNSUPPORTED, as said there — its rows cannot hold a set.  pcp_set_solution_sink, here, is the set-mode forests': every
 * solution of pcp_dfs_forest_device_set, _set_enum and _setform (both distributors), not only their number and the first one's lower
 * bounds.  A True node over IntervalSet domains is a PRODUCT OF SETS — every unit is entailed while a set may still hold several values and
 * may have holes — and every point of the product is a solution; neither the count nor first_solution says which points those are.  A row is
 * therefore the whole node, n_vars x set_words 64-bit words in the layout of a pcp_forest_state.bits row (bit b of word w of variable v:
 * the value hull_lo + 64 w + b).
 *   bits     : [capacity][n_vars][set_words] device uint64: row i = the i-th solution appended
 *   tree     : [capacity] device uint32 or NULL: the tree that wrote row i
 *   count    : device uint32: tickets drawn since the caller last zeroed it.  It may exceed capacity: the valid rows are min(*count, capacity)
 *   capacity : rows (> 0);  reserved : 0
 * It belongs to the context: the struct is copied at the call, the buffers stay the caller's, NULL detaches; the caller reads and zeroes
 * *count between launches, never during one.  pcp_model_reset DETACHES it, because the row width changes with the model.  (The Interval
 * sink survives pcp_model_reset: its attachment is left as it was, and its caller re-attaches after a reset that changes n_vars.)  It can
 * be attached to a set-mode context only (pcp_model_reset with set_words > 0), so the Interval entries never see one.
 * THE PROTOCOL is that of the Interval sink.  A node found to be a solution (not the StopNode limit node, which is none and draws no
 * ticket) draws slot = (*count)++ BEFORE it is counted.  slot < capacity: the node's sets go to row slot, tree[slot] = t, and the step goes
 * on as without a sink — counted, the forest's first solution kept, stop raised under stop_on_solution.  slot >= capacity: error 6, "sink
 * full", in counters[t][3] — nothing is counted, the node the tree reserved goes back to *total_nodes, the tree keeps the node as its
 * current node AT ITS FIXPOINT with tree[t][2] = PCP_DFS_FULL, trail and levels untouched, and *stop is raised (one word for all trees of
 * these forests): the contract of error 1 in this loop.  Errors 1, 3, 4 and 5 keep their meaning here.  A caller that copies the rows
 * out, zeroes *count, clears that tree's error word and *stop and calls again runs the node again — propagating a fixpoint narrows nothing
 * and trails nothing — and it is counted and appended then.  No counter of any tree differs from a run whose sink never fills: the
 * handed-back node was not counted and its reservation was returned; its second run leaves sets, trail and levels as the first did, so the
 * tree goes on from the state it would have had; the other trees see *stop between nodes only, as at any launch end, and a tree's nodes do
 * not depend on when they run.  No solution is lost or written twice; rows are in ticket order.  A tree stopped by error 6 is an ordinary
 * donor for pcp_dfs_forest_split_set.
 * pcp_dfs_forest_device_set_bnb and pcp_dfs_forest_device_setform_bnb return PCP_ERR_UNSUPPORTED and launch nothing while a set sink is
 * attached (branch and bound keeps tree_row); with none attached every entry launches exactly what it launched before.
 * A null bits or count, capacity == 0, reserved != 0, an interval-mode context: PCP_ERR_ARG, and the sink attached before stays. */
typedef struct {
  uint64_t* bits;
  uint32_t* tree;
  uint32_t* count;
  uint32_t capacity;
  uint32_t reserved;
} pcp_set_solution_sink;
int32_t pcp_set_solution_sink_set(pcp_ctx* ctx, const pcp_set_solution_sink* sink);
/* Between two calls of pcp_dfs_forest_device_set* / _setform*: finished trees take over work from trees that still have some.  pairs = n_pairs x
 * (donor, receiver) tree indices (device uint32).  For every pair whose receiver is finished and whose donor has an open right branch
 * left, the donor's OLDEST open right branch (the subtree nearest its root) becomes the receiver's new root — built from the donor's
 * current node and its trail — and done[pair] = 1; otherwise done[pair] = 0 and nothing changes.  The donor skips that branch when it
 * backtracks to it; counters are untouched, so the sum over the trees stays the search's.  A tree may appear in one pair per call.
 * tree[t][3] = finished (bit 0) | number of levels given away (bits 8..). */
int32_t pcp_dfs_forest_split_set(pcp_ctx* ctx, const pcp_forest_state* st, uint32_t n_pairs, const uint32_t* pairs, uint32_t* done, void* hip_stream);

/* Counters accumulate on the device across pcp_propagate_device calls.  pcp_stats_reset also clears the sticky hull-violation word;
 * pcp_stats_read is the only call that reports (and then clears) it. */
int32_t pcp_stats_reset(pcp_ctx* ctx, void* hip_stream);
int32_t pcp_stats_read(pcp_ctx* ctx, pcp_stats* out, void* hip_stream); /* synchronises hip_stream */

/* Diagnostics (ABI v6): kernel-internal event counters accumulated since the last pcp_stats_reset.  They describe HOW a launch got
 * to its result, never the result (the reference has no counterpart); tests use them to prove that a code path was taken.
 * out[0 .. n) receives the first n of PCP_DBG_COUNT counters (n <= PCP_DBG_COUNT); synchronises hip_stream. */
typedef enum {
  PCP_DBG_BIG_DENSE = 0,   /* path 2: wake-up rounds that streamed the record table again (one per node and round)            */
  PCP_DBG_BIG_SPARSE = 1,  /* path 2: wake-up rounds that walked the adjacency lists of the changed variables                  */
  PCP_DBG_NEQ_TILES = 2,   /* path 1: tiles run (a persistent workgroup runs several)                                         */
  PCP_DBG_NEQ_OVERLAP = 3, /* path 1: tiles whose rows were already in flight while the previous tile's rounds ran            */
  PCP_DBG_SMALL_NODES = 4, /* path 4: nodes run by the small-store kernel                                                     */
  PCP_DBG_NEQ_LEAN = 8,           /* path 1: tiles whose round 0 took the lean form (full 16-node tiles with at most four assigned variables) */
  PCP_DBG_NEQ_LEAN_PASSES = 9,    /* path 1: passes of that form beyond a tile's first (tiles in which a node narrowed)                      */
  PCP_DBG_NEQ_LEAN_HANDOVER = 10, /* path 1: lean tiles handed to the general rounds (a narrowing assigned or emptied a variable)              */
  PCP_DBG_COUNT = 16
} pcp_dbg_counter;
int32_t pcp_debug_counters(pcp_ctx* ctx, uint64_t* out, uint32_t n, void* hip_stream);

/* Timing of the LAST pcp_propagate_device call's kernels, measured with HIP events recorded on the
 * stream the kernels were launched on (bench.py's roofline leg).  Synchronises on the stop event. */
int32_t pcp_last_kernel_ms(pcp_ctx* ctx, float* ms);

/* The launch geometry the LAST pcp_propagate_device / pcp_propagate call chose (tests pin the benchmarked path to
 * the oracle by asserting on it; bench.py reports it). */
typedef struct {
  uint32_t nodes_per_block; /* B: nodes whose domains one workgroup keeps in LDS                       */
  uint32_t team;            /* workgroups cooperating on one node (1 = batch geometry)                 */
  uint32_t packed;          /* 1 = 16-bit packed LDS cells                                             */
  uint32_t word_level;      /* 0 = chunked record sweep, 1/2 = word-group sweep (level -1 range test)  */
  uint32_t global_dom;      /* 1 = domains stay in HBM (variable store larger than LDS); 2 = that variant with the domains in
                               LDS after all as 10-bit cells (declared hull of at most 1024 values)    */
  uint32_t compact;         /* 1 = 8-byte record stream                                                */
  uint32_t implicit_active; /* 1 = no `active` rows: liveness derived from the domains                 */
  uint32_t set_mode;        /* 1 = IntervalSet (bitset) domains                                        */
  uint32_t grid, block, lds_bytes, list_cap;
  uint32_t path;            /* 0 = the generic kernels (every propagator tested in the initial sweep, in bulk where range tests allow);
                               1 = the assignment-driven kernel of all-XNeqY models over implicit nodes: the sweep is the adjacency
                               lists of the assigned variables (an XNeqY between two unassigned variables is a no-op, x_neq_y.rs:82-93);
                               2 = the 10-bit-cell kernel of binary models whose store does not fit LDS as pairs (implicit nodes, declared hull);
                               3 = the formula kernel: a store with formula propagators (pcp_model_push_formula) or Boolean leaves (set_mode = 1: its
                                   IntervalSet form, pcp_setform.hip);
                               4 = the small-store kernel: at most 128 slots and 2048 elementary filters, one wavefront per node */
} pcp_plan;
int32_t pcp_last_plan(const pcp_ctx* ctx, pcp_plan* out);

/* Knobs (all optional; the defaults pick everything from the model and the batch).  key:
 *   "block_threads" 256/512/1024, "nodes_per_block" 0 = auto, "force_path" (0 auto, 1 batch LDS kernel, 2 team kernel),
 *   "team" workgroups per node, "list_cap" (the changed-variable list of a wake-up round, in LDS; 64..16384, default 2048; the interval kernels
 *   halve it until the store fits; set mode — pcp_propagate* on sets and pcp_dfs_forest_device_set* — uses min(list_cap, 1024), and a round
 *   with more changed variables than that sweeps every record instead), "global_dom" 1 = domains stay in HBM (2: 10-bit LDS cells allowed), "dom10" 0 = never use
 *   10-bit cells, "implicit_active" 0 = materialise rows for active_in NULL, "group_level" 0 = no group test, "packed" 0 = never use 16-bit cells,
 *   "word_level" 0 = never use the word-group sweep, "solo_cascade" 0 = a wake-up round with one changed variable is an ordinary round
 *   (1, the default: its records are re-run in place and a bound jumps over the values assigned neighbours forbid), "branch_reverse" 1 = pcp_branch_device writes child k of the batch
 *   to row n_children-1-k (a caller appending the rows to a LIFO stack then pops the first node's left child first), "var_select"
 *   PCP_VAR_FIRST_SMALLEST (0, the default) / PCP_VAR_INPUT_ORDER (1): the variable selector of every brancher and search loop (above, at
 *   the defines; any other value: PCP_ERR_ARG, the option keeps its value).
 * "time_kernels" 0 = no HIP events around the fixpoint launches: a call enqueues the kernel and nothing else, pcp_last_kernel_ms then has
 *   nothing to report (1, the default: two event records per launch, a few microseconds of queue time each), "small_path" 0 = small stores
 *   use the generic kernels too (1, the default: path 4; any option that asks for a geometry of the generic kernels — "nodes_per_block",
 *   "force_path", "team", "global_dom" — keeps them as well), "big_path" 0 = never use the 10-bit-cell kernel (path 2), "big_round" /
 *   "big_dense_k" its wake-up rounds (0 auto, 1 dense, 2 sparse; dense iff k * list entries >= records), "neq_persist" 0 = one workgroup
 *   per tile instead of persistent workgroups, "neq_dfs_block" threads per tree of the in-kernel search loop (0 = auto: 512 for one tree,
 *   256 for a forest), "neq_dfs" 0 = pcp_dfs_device launches one step at a time on all-XNeqY models too (1, the default: the whole search
 *   loop runs in one workgroup, n_steps nodes per launch), "neq_path" 0 = all-XNeqY models use the generic kernels too (1, the default: the
 *   assignment-driven kernel when the nodes are implicit), "neq_block" threads per workgroup of that kernel (0 = auto).
 *   (Rounds 3-4 had "neq_wave" / "neq_prefetch": two measured-and-rejected launch forms of the all-XNeqY kernel; their code left the
 *   library in round 5 — tools/micro/neq_rejected_r4.patch)
 * Unknown key -> PCP_ERR_ARG. */
int32_t pcp_set_option(pcp_ctx* ctx, const char* key, int64_t value);

#ifdef __cplusplus
}
#endif
#endif /* PCP_HIP_H */
