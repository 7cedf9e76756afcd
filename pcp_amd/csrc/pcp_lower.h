// pcp_lower.h — model lowering: from the pushed pcp_props to the tables the kernels read (pcp_tables.h).  Host arithmetic only:
// nothing here knows of HIP, so every encoding can be checked on a CPU (tests/lower_check.cpp).  pcp_api.hip uploads the results.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/pcp_hip.h"
#include "pcp_tables.h"

namespace pcp {

// The model as pushed through the C ABI (pcp_model_reset / _push_props / _push_sum / _push_formula / _truncate).
struct HostModel {
  uint32_t n_vars = 0;
  uint32_t set_words = 0;   // > 0: IntervalSet<i32> domains as bitsets (pcp_model_reset)
  std::vector<pcp_prop> props;          // as pushed
  std::vector<uint32_t> unit_of_prop;   // unit index of each prop
  std::vector<int32_t> formula_of_prop; // formula number of each prop (a leaf of that tree), or -1
  std::vector<std::vector<pcp_fnode>> formulas;  // pcp_model_push_formula: the trees (leaf.first = index among the formula's own leaves)
  std::vector<std::vector<uint32_t>> sums;  // term::Sum views: member variables of each term (pcp_model_push_sum)
  uint32_t n_units = 0;
  bool has_groups = false;
  bool has_formulas = false;            // a formula unit or a Boolean / BooleanNeg leaf: the store runs pcp_formula.hip (set mode: pcp_setform.hip)
  // The lowering is free of HIP and does not know which kernels its caller links.  Formula units and Boolean / BooleanNeg leaves over
  // IntervalSet stores (set_words > 0) need the set-mode formula kernel (pcp_setform.hip): a caller that has it says so here — pcp_ctx does —
  // and the validators then accept them; for any other caller they stay PCP_ERR_UNSUPPORTED, as before that kernel existed.
  bool set_formulas = false;
};

// What the launch code asks about a lowered model.
struct LoweredInfo {
  uint32_t n_slots = 0;              // n_vars + Sum slots + interned constants
  uint32_t n_sum_slots = 0;          // Sum terms with more than one member (those have a pseudo-slot)
  bool has_ternary = false;          // a record that is not binary, or a Sum view: generic path only
  uint32_t uniform_kind = 0xFFFFFFFFu;  // the kind shared by ALL records when that is NEQ or LT
  uint32_t max_deg = 0;              // longest adjacency list of a variable
  bool compact = false;              // recs8 present
  bool consts_fit16 = true;          // every interned constant within +-kPackedMax (packed tiles)
  uint32_t word_level = 0;           // 0 = no word descriptors worth using, 1 = XNeqY words only, 2 = XLessY words too
  bool neq_model = false;            // every record is an XNeqY with at least one variable operand, payload adjacency, slots < 65536
  bool have_adjp = false;
  bool have_adjp4 = false;           // 4-byte adjacency payloads (pcp_neq.hip)
  bool have_seed_always = false;     // variables with a Constant neighbour (pcp_neq.hip)
  uint32_t n_alldiff = 0;            // all-different units found (pcp_small.hip)
};

// The tables.  An optional table is empty when the model has none (its flag in LoweredInfo says the same).
struct Lowered : LoweredInfo {
  std::vector<Rec> recs;             // padded (kStreamPadRecs)
  std::vector<Rec8> recs8;           // padded alike; `compact`
  std::vector<WordDesc> wdesc;       // `word_level` != 0
  std::vector<GroupDesc> gdesc;      // with wdesc
  std::vector<uint32_t> adj_off, adj;
  std::vector<U32x2> adjp;           // ModelDev::adjp; `have_adjp`
  std::vector<uint32_t> adjp4;       // NeqArgs::adjp4; `have_adjp4`
  std::vector<uint32_t> seed_always; // NeqArgs::seed_always; `have_seed_always`
  std::vector<int32_t> consts;       // every slot >= n_vars (the Sum slots hold 0)
  std::vector<int32_t> mul_off;      // SumTab::mul_off
  std::vector<uint32_t> sum_off, sum_mem;  // SumTab; `n_sum_slots` != 0
  std::vector<uint32_t> unit_first;  // grouped models: first record of each unit (+ sentinel)
  // all-different units (pcp_small.hip): a Conjunction / Distinct unit whose members are x != y (no offsets, no constants) over EVERY pair of a
  // variable set of at most 64 variables — what Distinct::new builds (propagators/distinct.rs:63-83).  ad_tab = [n, then per unit: unit id,
  // count, first index into ad_vars]; ad_mask bit u = unit u is one.
  std::vector<uint32_t> ad_tab, ad_vars, ad_mask;  // `n_alldiff` != 0
  std::vector<pcp_fnode> fnodes;     // models with formulas: every unit as a tree (FormArgs, pcp_neq.h)
  std::vector<uint32_t> unit_root;
};

// Lowers the model.  Returns PCP_OK, or the error code with its text in `err` (`out` is then unspecified).
int32_t lower_model(const HostModel& m, Lowered& out, std::string& err);

// The table of pcp_big.hip (BigRec / BigAdj, pcp_neq.h) from the lowered tables: brec = the n_recs records sorted by kind (stable; with
// bank_order, reordered within a kind for LDS bank pairs) and padded like `recs`, badj = the payload of each adjacency entry.  False when
// the model does not fit the format — 98304 variables or more, an offset beyond +-4095, a constant that folds beyond +-2^30, a ternary
// kind, a record over two constants; the outputs are then unspecified.
bool lower_big(const std::vector<Rec>& recs, const std::vector<uint32_t>& adj_off, const std::vector<uint32_t>& adj, const std::vector<int32_t>& consts,
               uint32_t n_vars, uint32_t n_recs, bool bank_order, std::vector<U32x2>& brec, std::vector<U32x2>& badj);

// Reference-panic checks on one prop about to join the model (SURVEY.md §8b "Error conventions").
int32_t validate_prop(const HostModel& m, const pcp_prop& p, std::string& err);
// The same on a formula: the tree — children behind their parent and consecutive, every node reached exactly once, every leaf used exactly
// once, depth <= 8 — and then each leaf.
int32_t validate_formula(const HostModel& m, uint32_t n_nodes, const pcp_fnode* nodes, uint32_t n_leaves, const pcp_prop* leaves, std::string& err);

}  // namespace pcp
