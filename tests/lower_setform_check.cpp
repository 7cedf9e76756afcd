// lower_setform_check.cpp — CPU check of the model lowering (pcp_amd/csrc/pcp_lower.hip) for formula units in SET mode, built and run by
// tests/test_setform_cpu.py under AddressSanitizer and UBSan: a formula push lowers to the same trees and records whether the store holds
// Interval or IntervalSet domains (the expected tables are written out by hand), and what set mode cannot pin stays refused — XEqYMulZ and
// Sum operands, as props and as formula leaves.  The models declare HostModel::set_formulas as pcp_ctx does; without it the validators keep
// the refusal of formula units over sets.  The first mismatch ends the program with a non-zero status.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../pcp_amd/csrc/pcp_lower.h"

using namespace pcp;

#define CHECK(...)                                                           \
  do {                                                                       \
    if (!(__VA_ARGS__)) {                                                    \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #__VA_ARGS__);     \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

namespace {

using U32 = std::vector<uint32_t>;
using I32 = std::vector<int32_t>;
constexpr uint32_t C = PCP_CONST, NV = PCP_NOVAR;

pcp_prop prop(uint8_t kind, uint32_t x, int32_t ox, uint32_t y, int32_t oy, uint32_t z = NV, int32_t oz = 0) {
  return pcp_prop{kind, 0, 0, 0, {x, y, z}, {ox, oy, oz}};
}
bool is(const Rec& r, uint32_t kind, uint32_t x, uint32_t y, uint32_t z, int32_t d) { return r.xk == (x | kind << 28) && r.y == y && r.z == z && r.d == d; }
bool is(const pcp_fnode& n, uint8_t type, uint16_t n_children, uint32_t first) { return n.type == type && n.reserved == 0 && n.n_children == n_children && n.first == first; }

// what pcp_model_push_props / pcp_model_push_formula do to the model, validation included
void push(HostModel& m, const pcp_prop& p) {
  std::string err;
  CHECK(validate_prop(m, p, err) == PCP_OK);
  ++m.n_units;
  m.props.push_back(p);
  m.unit_of_prop.push_back(m.n_units - 1);
  m.formula_of_prop.push_back(-1);
  if (p.kind >= PCP_BOOL) m.has_formulas = true;
}
void push_formula(HostModel& m, const std::vector<pcp_fnode>& nodes, const std::vector<pcp_prop>& leaves) {
  std::string err;
  const int32_t rc = validate_formula(m, (uint32_t)nodes.size(), nodes.data(), (uint32_t)leaves.size(), leaves.data(), err);
  if (rc) { std::printf("FAIL validate_formula: %d %s\n", rc, err.c_str()); std::exit(1); }
  m.formulas.push_back(nodes);
  ++m.n_units;
  for (const pcp_prop& p : leaves) {
    m.props.push_back(p);
    m.unit_of_prop.push_back(m.n_units - 1);
    m.formula_of_prop.push_back((int32_t)m.formulas.size() - 1);
  }
  m.has_formulas = true;
}

// unit 0: x0 < x1 + 2;  unit 1: OR(x0 = 1, AND(x1 != x2 + 3, Boolean(x3)));  unit 2: BooleanNeg(x3 - 1);  unit 3: OR(x2 = 4, x0 = x1 + x2)
HostModel build(uint32_t set_words) {
  HostModel m;
  m.n_vars = 4;
  m.set_words = set_words;
  m.set_formulas = true;  // as pcp_ctx declares: the library has the set-mode formula kernel
  push(m, prop(PCP_LT, 0, 0, 1, 2));
  push_formula(m, {{PCP_F_OR, 0, 2, 1}, {PCP_F_LEAF, 0, 0, 0}, {PCP_F_AND, 0, 2, 3}, {PCP_F_LEAF, 0, 0, 1}, {PCP_F_LEAF, 0, 0, 2}},
               {prop(PCP_EQ, 0, 0, C, 1), prop(PCP_NEQ, 1, 0, 2, 3), prop(PCP_BOOL, 3, 0, NV, 0)});
  push(m, prop(PCP_NBOOL, 3, -1, NV, 0));
  push_formula(m, {{PCP_F_OR, 0, 2, 1}, {PCP_F_LEAF, 0, 0, 1}, {PCP_F_LEAF, 0, 0, 0}}, {prop(PCP_EQ3, 0, 0, 1, 0, 2, 0), prop(PCP_EQ, 2, 0, C, 4)});
  return m;
}

void same_tables() {
  Lowered lo[2];
  for (uint32_t k = 0; k < 2; ++k) {
    const HostModel m = build(k);
    CHECK(m.has_formulas && m.n_units == 4);
    std::string err;
    const int32_t rc = lower_model(m, lo[k], err);
    if (rc) { std::printf("FAIL lower_model (set_words %u): %d %s\n", k, rc, err.c_str()); std::exit(1); }
    const Lowered& l = lo[k];
    // records in push order; the constants 1 and 4 are interned as the slots n_vars = 4 and 5, as the set kernels expect
    CHECK(l.n_slots == 6 && l.n_sum_slots == 0 && (l.consts == I32{1, 4}));
    CHECK(is(l.recs[0], PCP_LT, 0, 1, 0, 2) && is(l.recs[1], PCP_EQ, 0, 4, 0, 0) && is(l.recs[2], PCP_NEQ, 1, 2, 0, 3));
    CHECK(is(l.recs[3], PCP_BOOL, 3, 0, 0, 0) && is(l.recs[4], PCP_NBOOL, 3, 0, 0, -1));
    CHECK(is(l.recs[5], PCP_EQ3, 0, 1, 2, 0) && is(l.recs[6], PCP_EQ, 2, 5, 0, 0));
    // every unit as a tree: a leaf's `first` is its record, an inner node's the index of its first child
    CHECK((l.unit_root == U32{0, 1, 6, 7, 10}) && l.fnodes.size() == 10);
    CHECK(is(l.fnodes[0], PCP_F_LEAF, 0, 0));
    CHECK(is(l.fnodes[1], PCP_F_OR, 2, 2) && is(l.fnodes[2], PCP_F_LEAF, 0, 1) && is(l.fnodes[3], PCP_F_AND, 2, 4));
    CHECK(is(l.fnodes[4], PCP_F_LEAF, 0, 2) && is(l.fnodes[5], PCP_F_LEAF, 0, 3));
    CHECK(is(l.fnodes[6], PCP_F_LEAF, 0, 4));
    CHECK(is(l.fnodes[7], PCP_F_OR, 2, 8) && is(l.fnodes[8], PCP_F_LEAF, 0, 6) && is(l.fnodes[9], PCP_F_LEAF, 0, 5));
  }
  // ... and the two lowerings agree entry for entry
  CHECK(lo[0].unit_root == lo[1].unit_root && lo[0].fnodes.size() == lo[1].fnodes.size() && lo[0].recs.size() == lo[1].recs.size());
  for (size_t i = 0; i < lo[0].fnodes.size(); ++i) CHECK(is(lo[1].fnodes[i], lo[0].fnodes[i].type, lo[0].fnodes[i].n_children, lo[0].fnodes[i].first));
  for (size_t i = 0; i < lo[0].recs.size(); ++i) CHECK(is(lo[1].recs[i], lo[0].recs[i].xk >> 28, lo[0].recs[i].xk & kSlotMask, lo[0].recs[i].y, lo[0].recs[i].z, lo[0].recs[i].d));
  // the limits carry over: a tree of 65 nodes that is no flat Conjunction
  std::vector<pcp_fnode> big{{PCP_F_AND, 0, 1, 1}, {PCP_F_OR, 0, 63, 2}};
  std::vector<pcp_prop> many;
  for (uint32_t i = 0; i < 63; ++i) { big.push_back({PCP_F_LEAF, 0, 0, i}); many.push_back(prop(PCP_NEQ, 0, 0, C, (int32_t)i)); }
  HostModel mb;
  mb.n_vars = 1; mb.set_words = 1; mb.set_formulas = true;
  push_formula(mb, big, many);
  Lowered out;
  std::string err;
  CHECK(lower_model(mb, out, err) == PCP_ERR_UNSUPPORTED && err == "a formula of more than 64 nodes (other than a flat Conjunction of propagators)");
  std::vector<pcp_fnode> deep;
  for (uint32_t i = 0; i < 9; ++i) deep.push_back({PCP_F_AND, 0, 1, i + 1});
  deep.push_back({PCP_F_LEAF, 0, 0, 0});
  CHECK(validate_formula(mb, 10, deep.data(), 1, many.data(), err) == PCP_ERR_UNSUPPORTED && err == "formula deeper than 8 levels");
  std::printf("ok formula tables in set mode\n");
}

void refusals() {
  HostModel m;
  m.n_vars = 4;
  m.set_words = 1;
  m.set_formulas = true;
  m.sums = {{0, 1}};
  std::string err;
  const char* mul = "XEqYMulZ over IntervalSet domains is not supported (interval mode only)";
  const char* sum = "Sum views over IntervalSet domains are not supported (interval mode only)";
  CHECK(validate_prop(m, prop(PCP_MUL3, 0, 0, 1, 0, 2, 0), err) == PCP_ERR_UNSUPPORTED && err == mul);
  CHECK(validate_prop(m, prop(PCP_LT, PCP_SUM | 0, 0, 2, 0), err) == PCP_ERR_UNSUPPORTED && err == sum);
  const std::vector<pcp_fnode> both{{PCP_F_OR, 0, 2, 1}, {PCP_F_LEAF, 0, 0, 0}, {PCP_F_LEAF, 0, 0, 1}};
  const std::vector<pcp_prop> with_mul{prop(PCP_BOOL, 3, 0, NV, 0), prop(PCP_MUL3, 0, 0, 1, 0, 2, 0)};
  const std::vector<pcp_prop> with_sum{prop(PCP_BOOL, 3, 0, NV, 0), prop(PCP_LT, PCP_SUM | 0, 0, 2, 0)};
  const std::vector<pcp_prop> fine{prop(PCP_BOOL, 3, 0, NV, 0), prop(PCP_LT, 0, 0, 2, 0)};
  CHECK(validate_formula(m, 3, both.data(), 2, with_mul.data(), err) == PCP_ERR_UNSUPPORTED && err == mul);
  CHECK(validate_formula(m, 3, both.data(), 2, with_sum.data(), err) == PCP_ERR_UNSUPPORTED && err == sum);
  CHECK(validate_formula(m, 3, both.data(), 2, fine.data(), err) == PCP_OK);
  CHECK(validate_prop(m, prop(PCP_BOOL, 3, 0, NV, 0), err) == PCP_OK && validate_prop(m, prop(PCP_NBOOL, 3, 0, NV, 0), err) == PCP_OK);
  // a caller without the set-mode formula kernel keeps the old refusal
  m.set_formulas = false;
  CHECK(validate_formula(m, 3, both.data(), 2, fine.data(), err) == PCP_ERR_UNSUPPORTED && err == "formula propagators are interval mode only");
  CHECK(validate_prop(m, prop(PCP_BOOL, 3, 0, NV, 0), err) == PCP_ERR_UNSUPPORTED && err == "the reified layer (Boolean / formulas) is interval mode only");
  // interval mode takes all of them
  m.set_words = 0;
  CHECK(validate_formula(m, 3, both.data(), 2, with_mul.data(), err) == PCP_OK && validate_formula(m, 3, both.data(), 2, with_sum.data(), err) == PCP_OK);
  std::printf("ok set-mode refusals\n");
}

}  // namespace

int main() {
  same_tables();
  refusals();
  std::printf("all ok\n");
  return 0;
}
