// lower_check.cpp — CPU check of the model lowering (pcp_amd/csrc/pcp_lower.hip), built and run by tests/test_lower_cpu.py under
// AddressSanitizer and UBSan.  Every expected value below is written out by hand from the format comments in pcp_tables.h and pcp_neq.h;
// none comes from running the lowering.  One line per case; the first mismatch ends the program with a non-zero status.
#include <algorithm>
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
constexpr uint32_t kNone = 0xFFFFFFFFu;

pcp_prop prop(uint8_t kind, uint32_t x, int32_t ox, uint32_t y, int32_t oy, uint32_t z = NV, int32_t oz = 0, uint8_t group_kind = 0, uint32_t group = 0) {
  return pcp_prop{kind, group_kind, 0, group, {x, y, z}, {ox, oy, oz}};
}
pcp_prop neq(uint32_t x, uint32_t y, uint8_t group_kind = 0, uint32_t group = 0) { return prop(PCP_NEQ, x, 0, y, 0, NV, 0, group_kind, group); }

// what pcp_model_push_props does to the model: a unit is a run of members of one call with the same group_kind and group
void push(HostModel& m, const std::vector<pcp_prop>& ps) {
  for (size_t i = 0; i < ps.size(); ++i) {
    const bool same = ps[i].group_kind != 0 && i > 0 && ps[i - 1].group_kind == ps[i].group_kind && ps[i - 1].group == ps[i].group;
    if (!same) ++m.n_units;
    if (ps[i].group_kind != 0) m.has_groups = true;
    m.props.push_back(ps[i]);
    m.unit_of_prop.push_back(m.n_units - 1);
    m.formula_of_prop.push_back(-1);
    if (ps[i].kind >= PCP_BOOL) m.has_formulas = true;
  }
}
// ... and pcp_model_push_formula
void push_formula(HostModel& m, const std::vector<pcp_fnode>& nodes, const std::vector<pcp_prop>& leaves) {
  m.formulas.push_back(nodes);
  ++m.n_units;
  for (const pcp_prop& p : leaves) {
    m.props.push_back(p);
    m.unit_of_prop.push_back(m.n_units - 1);
    m.formula_of_prop.push_back((int32_t)m.formulas.size() - 1);
  }
  m.has_formulas = true;
}
HostModel model(uint32_t n_vars, const std::vector<pcp_prop>& ps = {}) {
  HostModel m;
  m.n_vars = n_vars;
  push(m, ps);
  return m;
}
Lowered lower(const HostModel& m) {
  Lowered lo;
  std::string err;
  const int32_t rc = lower_model(m, lo, err);
  if (rc) { std::printf("FAIL lower_model: %d %s\n", rc, err.c_str()); std::exit(1); }
  return lo;
}
bool is(const Rec& r, uint32_t kind, uint32_t x, uint32_t y, uint32_t z, int32_t d) { return r.xk == (x | kind << 28) && r.y == y && r.z == z && r.d == d; }
bool is(const U32x2& p, uint32_t x, uint32_t y) { return p.x == x && p.y == y; }
bool is(const WordPart& p, uint32_t x, uint32_t y, uint32_t k, uint32_t d) { return p.x == x && p.y == y && p.k == k && p.d == d; }
bool is(const pcp_fnode& n, uint8_t type, uint16_t n_children, uint32_t first) { return n.type == type && n.reserved == 0 && n.n_children == n_children && n.first == first; }
bool zero(const WordPart& p) { return is(p, 0, 0, 0, 0); }
constexpr size_t kPad1 = 256 + kStreamPadRecs;  // padded length of a table of 1 .. 256 records

void records_and_constants() {
  // x0 < x1 + 2,  x1 != 5,  x0 + 1 = x1 + x2 - 3,  x2 != 5
  const Lowered lo = lower(model(3, {prop(PCP_LT, 0, 0, 1, 2), prop(PCP_NEQ, 1, 0, C, 5), prop(PCP_EQ3, 0, 1, 1, -3, 2, 0), prop(PCP_NEQ, 2, 0, C, 5)}));
  CHECK(lo.n_slots == 4 && lo.n_sum_slots == 0 && lo.consts == I32{5});  // both constants: the one slot n_vars = 3
  CHECK(is(lo.recs[0], PCP_LT, 0, 1, 0, 2));     // Y = y + d: d = 2 - 0
  CHECK(is(lo.recs[1], PCP_NEQ, 1, 3, 0, 0));    // a Constant's value is no offset
  CHECK(is(lo.recs[2], PCP_EQ3, 0, 1, 2, -4));   // x vs y + z + d: d = -3 + 0 - 1
  CHECK(is(lo.recs[3], PCP_NEQ, 2, 3, 0, 0));
  CHECK(lo.has_ternary && !lo.have_adjp && lo.adjp.empty() && lo.adjp4.empty() && lo.seed_always.empty());
  CHECK(!lo.compact && lo.recs8.empty() && lo.wdesc.empty() && lo.gdesc.empty() && lo.word_level == 0);
  CHECK(lo.uniform_kind == kNone && !lo.neq_model && !lo.have_adjp4 && !lo.have_seed_always && lo.consts_fit16);
  CHECK((lo.adj_off == U32{0, 2, 5, 7}) && (lo.adj == U32{0, 2, 0, 1, 2, 2, 3}) && lo.max_deg == 3);
  CHECK(lo.recs.size() == kPad1);
  for (size_t r = 4; r < lo.recs.size(); ++r) CHECK(is(lo.recs[r], PCP_NEQ, 2, 3, 0, 0));
  CHECK(lo.mul_off.empty() && lo.sum_off.empty() && lo.sum_mem.empty() && lo.unit_first.empty() && lo.ad_tab.empty() && lo.fnodes.empty() && lo.unit_root.empty());
  // an empty model: the CSR offsets only
  const Lowered e = lower(model(2));
  CHECK(e.recs.empty() && (e.adj_off == U32{0, 0, 0}) && e.adj.empty() && e.consts.empty() && e.n_slots == 2 && !e.compact);
  // XEqYMulZ: the three offsets go to the side table, d is the index
  const Lowered mu = lower(model(3, {prop(PCP_MUL3, 0, 1, 1, 2, 2, 3), prop(PCP_MUL3, 2, -1, 0, 0, 1, 4)}));
  CHECK(is(mu.recs[0], PCP_MUL3, 0, 1, 2, 0) && is(mu.recs[1], PCP_MUL3, 2, 0, 1, 1) && (mu.mul_off == I32{1, 2, 3, -1, 0, 4}));
  // constants beyond the packed tiles' range
  CHECK(!lower(model(1, {prop(PCP_NEQ, 0, 0, C, 16384)})).consts_fit16 && lower(model(1, {prop(PCP_NEQ, 0, 0, C, -16383)})).consts_fit16);
  std::printf("ok records and constants\n");
}

void sum_views() {
  HostModel m = model(3);
  m.sums = {{1}, {0, 2}};  // Sum 0 forwards to x1; Sum 1 = x0 + x2 gets the slot n_vars = 3
  push(m, {prop(PCP_LT, PCP_SUM | 0, 0, 0, 0), prop(PCP_NEQ, PCP_SUM | 1, 0, C, 7)});
  const Lowered lo = lower(m);
  CHECK(lo.n_sum_slots == 1 && lo.n_slots == 5 && (lo.consts == I32{0, 7}));  // the Sum slot holds 0, the constant comes behind it
  CHECK(is(lo.recs[0], PCP_LT, 1, 0, 0, 0) && is(lo.recs[1], PCP_NEQ, 3, 4, 0, 0));
  CHECK((lo.sum_off == U32{0, 2}) && (lo.sum_mem == U32{0, 2}));
  CHECK((lo.adj_off == U32{0, 2, 3, 4}) && (lo.adj == U32{0, 1, 0, 1}) && lo.max_deg == 2);  // both members of Sum 1 list record 1
  CHECK(lo.has_ternary && lo.uniform_kind == kNone && !lo.have_adjp && !lo.compact);
  std::printf("ok sum views\n");
}

void binary_payloads() {
  // x0 != x1 + 3,  x2 + 1 != x0,  x1 != 9
  const std::vector<pcp_prop> ps{prop(PCP_NEQ, 0, 0, 1, 3), prop(PCP_NEQ, 2, 1, 0, 0), prop(PCP_NEQ, 1, 0, C, 9)};
  const Lowered lo = lower(model(3, ps));
  CHECK(is(lo.recs[0], PCP_NEQ, 0, 1, 0, 3) && is(lo.recs[1], PCP_NEQ, 2, 0, 0, -1) && is(lo.recs[2], PCP_NEQ, 1, 3, 0, 0));
  CHECK((lo.adj_off == U32{0, 2, 4, 5}) && (lo.adj == U32{0, 1, 0, 2, 1}));
  CHECK(!lo.has_ternary && lo.have_adjp && lo.uniform_kind == PCP_NEQ && lo.neq_model && lo.have_adjp4 && lo.have_seed_always && lo.compact);
  const uint32_t Y = 1u << 31;  // this variable is the record's y
  CHECK(lo.adjp.size() == 5);
  CHECK(is(lo.adjp[0], 1, 3) && is(lo.adjp[1], 2 | Y, 0xFFFFFFFFu));  // x0: record 0 as x, record 1 as y
  CHECK(is(lo.adjp[2], 0 | Y, 3) && is(lo.adjp[3], 3, 0));            // x1: record 0 as y, record 2 against the constant's slot
  CHECK(is(lo.adjp[4], 0, 0xFFFFFFFFu));                              // x2: record 1 as x
  // other | is_y << 15 | t << 16 with t = -d on the x side, d on the y side
  // ... and one zero entry behind the last list
  CHECK((lo.adjp4 == U32{1u | 0xFFFDu << 16, 2u | 1u << 15 | 0xFFFFu << 16, 0u | 1u << 15 | 3u << 16, 3u, 0u | 1u << 16, 0u}));
  CHECK(lo.seed_always == U32{1u << 1});  // x1 is the constant's only neighbour
  // the kind travels in bits 28..30
  std::vector<pcp_prop> lt = ps;
  lt[0].kind = PCP_LT;
  const Lowered l2 = lower(model(3, lt));
  CHECK(l2.have_adjp && is(l2.adjp[0], 1 | 2u << 28, 3) && is(l2.adjp[2], 0 | 2u << 28 | Y, 3) && is(l2.adjp[3], 3, 0));
  CHECK(l2.uniform_kind == kNone && !l2.neq_model && !l2.have_adjp4 && !l2.have_seed_always && l2.adjp4.empty() && l2.seed_always.empty());
  // a record over two constants: no variable's list would run it
  std::vector<pcp_prop> cc = ps;
  cc.push_back(prop(PCP_NEQ, C, 9, C, 4));
  const Lowered l3 = lower(model(3, cc));
  CHECK(is(l3.recs[3], PCP_NEQ, 3, 4, 0, 0) && (l3.consts == I32{9, 4}));
  CHECK(l3.uniform_kind == PCP_NEQ && l3.have_adjp && !l3.neq_model && !l3.have_adjp4 && !l3.have_seed_always);
  // an offset that does not fit int16
  std::vector<pcp_prop> wide = ps;
  wide[0].off[1] = 32768;
  const Lowered l4 = lower(model(3, wide));
  CHECK(l4.neq_model && !l4.have_adjp4 && l4.adjp4.empty() && l4.have_seed_always && is(l4.adjp[0], 1, 32768));
  wide[0].off[1] = 32767;
  CHECK(lower(model(3, wide)).have_adjp4);
  // a last variable that is in no record (x3): its empty list starts at adj_off[n_vars], the end of the payloads.  The lean round 0 of pcp_neq.hip
  // requests a listed variable's first entry whatever its degree (neq_fast_load): the 4-byte table keeps one zero entry there.
  const Lowered iso = lower(model(4, {prop(PCP_NEQ, 0, 0, 1, 3), prop(PCP_NEQ, 2, 1, 0, 0)}));
  CHECK((iso.adj_off == U32{0, 2, 3, 4, 4}) && iso.adj.size() == 4 && iso.adjp.size() == 4 && iso.neq_model && iso.have_adjp4 && !iso.have_seed_always);
  CHECK(iso.adjp4.size() == iso.adj_off[4] + 1 && iso.adjp4.back() == 0u);
  CHECK((iso.adjp4 == U32{1u | 0xFFFDu << 16, 2u | 1u << 15 | 0xFFFFu << 16, 0u | 1u << 15 | 3u << 16, 0u | 1u << 16, 0u}));
  std::printf("ok binary model payloads\n");
}

// 128 x_i != x_j records in two words (see word_descriptors)
std::vector<pcp_prop> two_words() {
  std::vector<pcp_prop> ps;
  for (uint32_t i = 0; i < 64; ++i) ps.push_back(neq(i / 16, 4 + i % 37));  // word 0: x in [0, 3], y in [4, 40]
  ps[0].off[0] = 2;  // d = -2
  ps[1].off[1] = 5;  // d = 5
  for (uint32_t i = 0; i < 20; ++i) ps.push_back(neq(10, 100 + i));  // word 1: x = 10 with y in [100, 119], then
  for (uint32_t i = 0; i < 44; ++i) ps.push_back(neq(11, 12 + i));   //         x = 11 with y back in [12, 55]
  return ps;
}

void word_descriptors() {
  std::vector<pcp_prop> ps = two_words();
  const Lowered lo = lower(model(120, ps));
  CHECK(lo.compact && lo.word_level == 1 && lo.wdesc.size() == 2 + kStreamPadRecs / 64);
  // word 0: 4 x slots -> level 2, second_x = 3 - 4 + 1; 37 y slots -> level 5, second_y = 40 - 32 + 1; cls 1; d in [-2, 5]
  CHECK(is(lo.wdesc[0].a, 0u | 0u << 16, 4u | 9u << 16, 2u | 5u << 4 | 1u << 8, 0xFFFEu | 5u << 16) && zero(lo.wdesc[0].b));
  // word 1: as one part its y slots span 108; two parts.  a: x = 10 (level 0), 20 y slots -> level 4, second_y = 119 - 16 + 1, bit 12
  CHECK(is(lo.wdesc[1].a, 10u | 10u << 16, 100u | 104u << 16, 0u | 4u << 4 | 1u << 8 | 1u << 12, 0));
  //         b: x = 11, 44 y slots -> level 5, second_y = 55 - 32 + 1
  CHECK(is(lo.wdesc[1].b, 11u | 11u << 16, 12u | 24u << 16, 0u | 5u << 4 | 1u << 8, 0));
  for (size_t w = 2; w < lo.wdesc.size(); ++w) CHECK(zero(lo.wdesc[w].a) && zero(lo.wdesc[w].b));
  // the one group: x in [0, 11] -> level 3, second_x = 11 - 8 + 1; smallest y 4; d in [-2, 5]
  CHECK(lo.gdesc.size() == 1 && lo.gdesc[0].x == (0u | 4u << 16) && lo.gdesc[0].k == (3u | 1u << 8) && lo.gdesc[0].ylo == 4 && lo.gdesc[0].d == (0xFFFEu | 5u << 16));
  // word 1 as XLessY: maximum tables as well
  for (size_t r = 64; r < 128; ++r) ps[r].kind = PCP_LT;
  const Lowered lt = lower(model(120, ps));
  CHECK(lt.word_level == 2 && lt.wdesc[1].a.k == (0u | 4u << 4 | 2u << 8 | 1u << 12) && lt.wdesc[1].b.k == (0u | 5u << 4 | 2u << 8) && lt.wdesc[0].a.k == (2u | 5u << 4 | 1u << 8));
  CHECK(lt.gdesc.size() == 1 && lt.gdesc[0].k == 0);  // a group of two kinds has no group test
  // word 0 with an x range of 64 slots: no descriptor, the word always goes to the record-level tests
  ps = two_words();
  ps[2].var[0] = 64;
  const Lowered far = lower(model(120, ps));
  CHECK(far.word_level == 1 && zero(far.wdesc[0].a) && zero(far.wdesc[0].b) && far.wdesc[1].a.k == (0u | 4u << 4 | 1u << 8 | 1u << 12));
  // fewer than half the words qualify: no word-level sweep
  ps[64].var[0] = 119;
  ps[64].var[1] = 0;  // word 1: x = 119, 10, 11 — the split at the first change of x leaves a second part that jumps
  const Lowered none = lower(model(120, ps));
  CHECK(none.compact && none.word_level == 0 && none.wdesc.empty() && none.gdesc.empty());
  std::printf("ok word descriptors\n");
}

void rec8() {
  const Lowered lo = lower(model(32768, {prop(PCP_LT, 5, 0, 32767, 7)}));
  CHECK(lo.compact && lo.n_slots == kCompactSlots && lo.recs8.size() == kPad1);
  for (const Rec8& r : lo.recs8) CHECK(r.xyk == (5u | 32767u << 15 | 2u << 30) && r.d == 7);
  CHECK(!lower(model(32768, {prop(PCP_LT, 5, 0, C, 7)})).compact);  // one slot more
  std::printf("ok Rec8\n");
}

std::vector<pcp_prop> distinct(const U32& vars, uint32_t group) {
  std::vector<pcp_prop> ps;
  for (size_t i = 0; i < vars.size(); ++i)
    for (size_t j = i + 1; j < vars.size(); ++j) ps.push_back(neq(vars[i], vars[j], 2, group));
  return ps;
}

void alldiff() {
  std::vector<pcp_prop> ps{neq(4, 5)};  // unit 0, standalone
  const std::vector<pcp_prop> d4 = distinct({0, 1, 2, 3}, 1);  // unit 1: 6 pairs
  ps.insert(ps.end(), d4.begin(), d4.end());
  const Lowered lo = lower(model(6, ps));
  CHECK(lo.n_alldiff == 1 && (lo.ad_tab == U32{1, 1, 4, 0}) && (lo.ad_vars == U32{0, 1, 2, 3}) && (lo.ad_mask == U32{1u << 1}));
  CHECK(lo.unit_first == U32{0, 1, 7});
  std::vector<pcp_prop> less = ps;
  less.pop_back();  // the pair (2, 3) is missing
  const Lowered l2 = lower(model(6, less));
  CHECK(l2.n_alldiff == 0 && l2.ad_tab.empty() && l2.ad_vars.empty() && l2.ad_mask.empty() && (l2.unit_first == U32{0, 1, 6}));
  std::vector<pcp_prop> off = ps;
  off[3].off[1] = 1;
  CHECK(lower(model(6, off)).n_alldiff == 0);
  // nine qualifying units of three variables each: the kernel keeps eight
  std::vector<pcp_prop> nine;
  for (uint32_t u = 0; u < 9; ++u) { const std::vector<pcp_prop> d = distinct({3 * u, 3 * u + 1, 3 * u + 2}, u); nine.insert(nine.end(), d.begin(), d.end()); }
  const Lowered l9 = lower(model(27, nine));
  CHECK(l9.n_alldiff == 8 && l9.ad_tab.size() == 25 && l9.ad_tab[0] == 8 && l9.ad_vars.size() == 24 && (l9.ad_mask == U32{0xFFu}));
  for (uint32_t u = 0; u < 8; ++u) CHECK(l9.ad_tab[1 + 3 * u] == u && l9.ad_tab[2 + 3 * u] == 3 && l9.ad_tab[3 + 3 * u] == 3 * u && l9.ad_vars[3 * u + 2] == 3 * u + 2);
  std::printf("ok all-different detection\n");
}

void formula_trees() {
  HostModel m = model(4);
  push(m, {prop(PCP_LT, 0, 0, 1, 0)});                               // unit 0: record 0
  push(m, {neq(0, 1, 1, 7), neq(0, 2, 1, 7), neq(1, 2, 1, 7)});      // unit 1: records 1..3
  const std::vector<pcp_prop> leaves{prop(PCP_EQ, 0, 0, C, 1), prop(PCP_EQ, 1, 0, C, 2), prop(PCP_EQ, 2, 0, C, 3)};
  // OR(leaf 0, AND(leaf 1, leaf 2))                                 // unit 2: records 4..6, nodes from 5
  push_formula(m, {{PCP_F_OR, 0, 2, 1}, {PCP_F_LEAF, 0, 0, 0}, {PCP_F_AND, 0, 2, 3}, {PCP_F_LEAF, 0, 0, 1}, {PCP_F_LEAF, 0, 0, 2}}, leaves);
  const Lowered lo = lower(m);
  CHECK(lo.fnodes.size() == 10 && (lo.unit_root == U32{0, 1, 5, 10}) && lo.n_alldiff == 0 && (lo.unit_first == U32{0, 1, 4, 7}));
  CHECK(is(lo.fnodes[0], PCP_F_LEAF, 0, 0));
  CHECK(is(lo.fnodes[1], PCP_F_AND, 3, 2) && is(lo.fnodes[2], PCP_F_LEAF, 0, 1) && is(lo.fnodes[3], PCP_F_LEAF, 0, 2) && is(lo.fnodes[4], PCP_F_LEAF, 0, 3));
  CHECK(is(lo.fnodes[5], PCP_F_OR, 2, 6) && is(lo.fnodes[6], PCP_F_LEAF, 0, 4) && is(lo.fnodes[7], PCP_F_AND, 2, 8));
  CHECK(is(lo.fnodes[8], PCP_F_LEAF, 0, 5) && is(lo.fnodes[9], PCP_F_LEAF, 0, 6));
  // 65 nodes, not flat: AND(OR(63 leaves))
  std::vector<pcp_fnode> big{{PCP_F_AND, 0, 1, 1}, {PCP_F_OR, 0, 63, 2}};
  std::vector<pcp_prop> many;
  for (uint32_t i = 0; i < 63; ++i) { big.push_back({PCP_F_LEAF, 0, 0, i}); many.push_back(prop(PCP_NEQ, 0, 0, C, (int32_t)i)); }
  HostModel mb = model(1);
  std::string err;
  CHECK(validate_formula(mb, 65, big.data(), 63, many.data(), err) == PCP_OK);
  push_formula(mb, big, many);
  Lowered out;
  CHECK(lower_model(mb, out, err) == PCP_ERR_UNSUPPORTED && err == "a formula of more than 64 nodes (other than a flat Conjunction of propagators)");
  // ... while a flat Conjunction may be wider
  std::vector<pcp_fnode> flat{{PCP_F_AND, 0, 65, 1}};
  many.clear();
  for (uint32_t i = 0; i < 65; ++i) { flat.push_back({PCP_F_LEAF, 0, 0, i}); many.push_back(prop(PCP_NEQ, 0, 0, C, (int32_t)i)); }
  HostModel mf = model(1);
  push_formula(mf, flat, many);
  const Lowered lf = lower(mf);
  CHECK(lf.fnodes.size() == 66 && (lf.unit_root == U32{0, 66}) && is(lf.fnodes[0], PCP_F_AND, 65, 1) && is(lf.fnodes[65], PCP_F_LEAF, 0, 64));
  // a Conjunction of 65 536 members next to a formula
  HostModel mc = model(2);
  push(mc, std::vector<pcp_prop>(65536, prop(PCP_LT, 0, 0, 1, 0, NV, 0, 1, 0)));
  push(mc, {prop(PCP_BOOL, 0, 0, NV, 0)});
  CHECK(lower_model(mc, out, err) == PCP_ERR_UNSUPPORTED && err == "a Conjunction of more than 65535 members next to formula propagators");
  // the folded offset of a record
  CHECK(lower_model(model(2, {prop(PCP_EQ, 0, -PCP_BOUND_MAX, 1, PCP_BOUND_MAX)}), out, err) == PCP_ERR_CONTRACT && err == "folded offset outside +-PCP_BOUND_MAX");
  std::printf("ok formula trees\n");
}

uint32_t cell(uint32_t word, uint32_t field) { return word | field << 15; }  // slot s lives in word s / 3, field s % 3

void big_tables() {
  // slots 0..6 variables, 7 = the constant 10, 8 = the constant 20
  const std::vector<pcp_prop> ps{
      prop(PCP_LT, 0, 0, 4, 1),       // r0  x0 < x4 + 1
      prop(PCP_NEQ, 1, 2, 5, 0),      // r1  x1 + 2 != x5          d = -2
      prop(PCP_EQ, 2, 0, 3, 0),       // r2  x2 = x3
      prop(PCP_NEQ, 3, 2, C, 10),     // r3  x3 + 2 != 10          x (kind) K: x3 != 8
      prop(PCP_LT, C, 20, 6, 3),      // r4  20 < x6 + 3           K (kind) y: x6 > 17
      prop(PCP_NEQ, 4, 0, 0, 0),      // r5  x4 != x0
      prop(PCP_LT, 5, 4095, 6, 0),    // r6  x5 + 4095 < x6        d = -4095
      prop(PCP_EQ, 6, 0, 1, 4095)};   // r7  x6 = x1 + 4095
  const Lowered lo = lower(model(7, ps));
  CHECK(lo.n_slots == 9 && (lo.consts == I32{10, 20}) && (lo.adj_off == U32{0, 2, 4, 5, 7, 9, 11, 14}));
  CHECK((lo.adj == U32{0, 5, 1, 7, 2, 2, 3, 0, 5, 1, 6, 4, 6, 7}));
  std::vector<U32x2> brec, badj;
  CHECK(lower_big(lo.recs, lo.adj_off, lo.adj, lo.consts, 7, 8, false, brec, badj));
  // BigRec: word_x | field_x << 15 | (d & 0x1fff) << 17 | kind << 30,  word_y | field_y << 15; a record with a Constant: kind 3, the op in the d field, K.
  // Stable by kind: NEQ r1 r5, EQ r2 r7, LT r0 r6, unary r3 r4.
  CHECK(brec.size() == kPad1);
  CHECK(is(brec[0], cell(0, 1) | 0x1FFEu << 17, cell(1, 2)) && is(brec[1], cell(1, 1), cell(0, 0)));
  CHECK(is(brec[2], cell(0, 2) | 1u << 30, cell(1, 0)) && is(brec[3], cell(2, 0) | 4095u << 17 | 1u << 30, cell(0, 1)));
  CHECK(is(brec[4], cell(0, 0) | 1u << 17 | 2u << 30, cell(1, 1)) && is(brec[5], cell(1, 2) | 0x1001u << 17 | 2u << 30, cell(2, 0)));
  CHECK(is(brec[6], cell(1, 0) | 3u << 17 | 3u << 30, 8) && is(brec[7], cell(2, 0) | 1u << 17 | 3u << 30, 17));
  for (size_t r = 8; r < brec.size(); ++r) CHECK(is(brec[r], brec[7].x, brec[7].y));
  // BigAdj, in the order of adj: word_other | field_other << 15 | is_y << 17 | kind << 18,  d; a unary record: 0x7fff | op << 18 | 1 << 20,  K
  const uint32_t Y = 1u << 17, U = 0x7FFFu | 1u << 20, m2 = (uint32_t)-2, m4095 = (uint32_t)-4095;
  const std::vector<U32x2> want{
      {cell(1, 1) | 2u << 18, 1}, {cell(1, 1) | Y, 0},                                                    // x0: r0 (x), r5 (y)
      {cell(1, 2), m2}, {cell(2, 0) | Y | 1u << 18, 4095},                                                // x1: r1 (x), r7 (y)
      {cell(1, 0) | 1u << 18, 0},                                                                         // x2: r2 (x)
      {cell(0, 2) | Y | 1u << 18, 0}, {U | 3u << 18, 8},                                                  // x3: r2 (y), r3
      {cell(0, 0) | Y | 2u << 18, 1}, {cell(0, 0), 0},                                                    // x4: r0 (y), r5 (x)
      {cell(0, 1) | Y, m2}, {cell(2, 0) | 2u << 18, m4095},                                               // x5: r1 (y), r6 (x)
      {U | 1u << 18, 17}, {cell(1, 2) | Y | 2u << 18, m4095}, {cell(0, 1) | 1u << 18, 4095}};             // x6: r4, r6 (y), r7 (x)
  CHECK(badj.size() == want.size());
  for (size_t k = 0; k < want.size(); ++k) CHECK(is(badj[k], want[k].x, want[k].y));
  // bank order: the same records within each kind's run, the same payloads
  std::vector<U32x2> brec2, badj2;
  CHECK(lower_big(lo.recs, lo.adj_off, lo.adj, lo.consts, 7, 8, true, brec2, badj2));
  CHECK(brec2.size() == brec.size() && badj2.size() == badj.size());
  for (size_t k = 0; k < badj.size(); ++k) CHECK(is(badj2[k], badj[k].x, badj[k].y));
  auto key = [](const U32x2& p) { return (uint64_t)p.x << 32 | p.y; };
  for (size_t s = 0; s < 8; s += 2) {
    std::vector<uint64_t> a{key(brec[s]), key(brec[s + 1])}, b{key(brec2[s]), key(brec2[s + 1])};
    std::sort(a.begin(), a.end());
    std::sort(b.begin(), b.end());
    CHECK(a == b);
  }
  for (size_t r = 8; r < brec2.size(); ++r) CHECK(is(brec2[r], brec2[7].x, brec2[7].y));
  // what the format cannot hold
  const U32 off1{0, 1}, adj1{0};
  const std::vector<Rec> fold{{0u | (uint32_t)PCP_NEQ << 28, 1, 0, 1}};  // x0 != K with K = 2^30 + 1
  CHECK(!lower_big(fold, off1, adj1, I32{1 << 30}, 1, 1, false, brec, badj));
  CHECK(lower_big(fold, off1, adj1, I32{(1 << 30) - 1}, 1, 1, false, brec, badj) && is(brec[0], cell(0, 0) | 3u << 17 | 3u << 30, 1u << 30));
  const std::vector<Rec> back{{1u | (uint32_t)PCP_NEQ << 28, 0, 0, 1}};  // K != x0 + 1 with K = -2^30: x0 != -2^30 - 1
  CHECK(!lower_big(back, off1, adj1, I32{-(1 << 30)}, 1, 1, false, brec, badj));
  const Lowered wide = lower(model(2, {prop(PCP_LT, 0, 0, 1, 4096)}));
  CHECK(!lower_big(wide.recs, wide.adj_off, wide.adj, wide.consts, 2, 1, false, brec, badj));
  const Lowered fits = lower(model(2, {prop(PCP_LT, 0, 4095, 1, 0)}));
  CHECK(lower_big(fits.recs, fits.adj_off, fits.adj, fits.consts, 2, 1, true, brec, badj));
  const Lowered cc = lower(model(2, {neq(0, 1), prop(PCP_NEQ, C, 1, C, 2)}));
  CHECK(!lower_big(cc.recs, cc.adj_off, cc.adj, cc.consts, 2, 2, false, brec, badj));
  const Lowered tern = lower(model(3, {prop(PCP_LT3, 0, 0, 1, 0, 2, 0)}));
  CHECK(!lower_big(tern.recs, tern.adj_off, tern.adj, tern.consts, 3, 1, false, brec, badj));
  std::printf("ok lower_big\n");
}

void expect(int32_t rc, const std::string& err, int32_t code, const char* msg, int line) {
  if (rc != code || err != msg) {
    std::printf("FAIL %s:%d: got %d \"%s\", expected %d \"%s\"\n", __FILE__, line, rc, err.c_str(), code, msg);
    std::exit(1);
  }
}
#define EXPECT_PROP(m, p, code, msg) do { std::string e_; expect(validate_prop(m, p, e_), e_, code, msg, __LINE__); } while (0)
#define EXPECT_FORMULA(m, nodes, leaves, code, msg)                                                                                           \
  do {                                                                                                                                        \
    std::string e_;                                                                                                                           \
    expect(validate_formula(m, (uint32_t)nodes.size(), nodes.data(), (uint32_t)leaves.size(), leaves.data(), e_), e_, code, msg, __LINE__);  \
  } while (0)

void validators() {
  HostModel m = model(3);
  m.sums = {{0, 1}};
  HostModel sets = m;
  sets.set_words = 1;
  std::string err;
  CHECK(validate_prop(m, prop(PCP_EQ3, 0, 1, 1, -1, 2, 0), err) == PCP_OK && validate_prop(m, prop(PCP_LT, PCP_SUM | 0, 0, 2, 0), err) == PCP_OK);
  EXPECT_PROP(m, prop(9, 0, 0, 1, 0), PCP_ERR_ARG, "unknown propagator kind");
  EXPECT_PROP(sets, prop(PCP_BOOL, 0, 0, NV, 0), PCP_ERR_UNSUPPORTED, "the reified layer (Boolean / formulas) is interval mode only");
  EXPECT_PROP(m, prop(PCP_NEQ, 0, 0, 1, 0, NV, 0, 3), PCP_ERR_ARG, "bad group_kind/reserved");
  pcp_prop res = neq(0, 1);
  res.reserved = 1;
  EXPECT_PROP(m, res, PCP_ERR_ARG, "bad group_kind/reserved");
  EXPECT_PROP(m, prop(PCP_NEQ, 0, 0, NV, 0), PCP_ERR_ARG, "missing operand");
  EXPECT_PROP(m, prop(PCP_NEQ, 0, 0, 1, PCP_BOUND_MAX + 1), PCP_ERR_CONTRACT, "offset outside +-PCP_BOUND_MAX");
  EXPECT_PROP(m, prop(PCP_NEQ, 0, -PCP_BOUND_MAX - 1, 1, 0), PCP_ERR_CONTRACT, "offset outside +-PCP_BOUND_MAX");
  EXPECT_PROP(m, prop(PCP_NEQ, PCP_SUM | 1, 0, 2, 0), PCP_ERR_ARG, "unknown Sum term (pcp_model_push_sum)");
  EXPECT_PROP(sets, prop(PCP_NEQ, PCP_SUM | 0, 0, 2, 0), PCP_ERR_UNSUPPORTED, "Sum views over IntervalSet domains are not supported (interval mode only)");
  EXPECT_PROP(m, prop(PCP_MUL3, 2, 0, PCP_SUM | 0, 0, C, 2), PCP_ERR_UNSUPPORTED, "XEqYMulZ over a Sum view is not supported");
  EXPECT_PROP(m, prop(PCP_NEQ, 0, 0, 3, 0), PCP_ERR_CONTRACT, "variable index out of range (variable/store.rs:176-179)");
  EXPECT_PROP(m, prop(PCP_NEQ, 1, 0, 1, 2), PCP_ERR_CONTRACT, "propagator already subscribed to this variable (reactors/indexed_deps.rs:69-77)");
  EXPECT_PROP(m, prop(PCP_LT, PCP_SUM | 0, 0, 1, 0), PCP_ERR_CONTRACT, "propagator already subscribed to this variable (reactors/indexed_deps.rs:69-77)");
  EXPECT_PROP(sets, prop(PCP_MUL3, 0, 0, 1, 0, 2, 0), PCP_ERR_UNSUPPORTED, "XEqYMulZ over IntervalSet domains is not supported (interval mode only)");

  const std::vector<pcp_prop> one{neq(0, 1)}, two{neq(0, 1), neq(1, 2)};
  using Nodes = std::vector<pcp_fnode>;
  const Nodes leaf{{PCP_F_LEAF, 0, 0, 0}}, both{{PCP_F_OR, 0, 2, 1}, {PCP_F_LEAF, 0, 0, 1}, {PCP_F_LEAF, 0, 0, 0}};
  EXPECT_FORMULA(m, leaf, one, PCP_OK, "");
  EXPECT_FORMULA(m, both, two, PCP_OK, "");
  EXPECT_FORMULA(sets, leaf, one, PCP_ERR_UNSUPPORTED, "formula propagators are interval mode only");
  const Nodes bad_type{{3, 0, 0, 0}}, bad_res{{PCP_F_LEAF, 1, 0, 0}};
  EXPECT_FORMULA(m, bad_type, one, PCP_ERR_ARG, "bad formula node");
  EXPECT_FORMULA(m, bad_res, one, PCP_ERR_ARG, "bad formula node");
  const Nodes orphan{{PCP_F_AND, 0, 1, 1}, {PCP_F_LEAF, 0, 0, 0}, {PCP_F_LEAF, 0, 0, 0}};
  EXPECT_FORMULA(m, orphan, one, PCP_ERR_ARG, "formula node not reached exactly once from the root");
  Nodes deep;
  for (uint32_t i = 0; i < 9; ++i) deep.push_back({PCP_F_AND, 0, 1, i + 1});
  deep.push_back({PCP_F_LEAF, 0, 0, 0});
  EXPECT_FORMULA(m, deep, one, PCP_ERR_UNSUPPORTED, "formula deeper than 8 levels");
  Nodes ok8;  // eight levels: seven inner nodes above the leaf
  for (uint32_t i = 0; i < 7; ++i) ok8.push_back({PCP_F_AND, 0, 1, i + 1});
  ok8.push_back({PCP_F_LEAF, 0, 0, 0});
  EXPECT_FORMULA(m, ok8, one, PCP_OK, "");
  const Nodes far_leaf{{PCP_F_LEAF, 0, 0, 1}};
  EXPECT_FORMULA(m, far_leaf, one, PCP_ERR_ARG, "formula leaf out of range");
  const Nodes twice{{PCP_F_AND, 0, 2, 1}, {PCP_F_LEAF, 0, 0, 0}, {PCP_F_LEAF, 0, 0, 0}};
  EXPECT_FORMULA(m, twice, one, PCP_ERR_ARG, "formula leaf used twice");
  const Nodes childless{{PCP_F_AND, 0, 0, 1}};
  EXPECT_FORMULA(m, childless, one, PCP_ERR_CONTRACT, "a Conjunction / Disjunction needs at least one child");
  const Nodes beyond{{PCP_F_AND, 0, 2, 1}, {PCP_F_LEAF, 0, 0, 0}}, backwards{{PCP_F_AND, 0, 1, 0}};
  EXPECT_FORMULA(m, beyond, one, PCP_ERR_ARG, "formula children out of range");
  EXPECT_FORMULA(m, backwards, one, PCP_ERR_ARG, "formula children out of range");
  EXPECT_FORMULA(m, leaf, two, PCP_ERR_ARG, "formula leaf not used");
  const std::vector<pcp_prop> bad_leaf{neq(0, 3)};
  EXPECT_FORMULA(m, leaf, bad_leaf, PCP_ERR_CONTRACT, "variable index out of range (variable/store.rs:176-179)");
  std::printf("ok validators\n");
}

}  // namespace

int main() {
  records_and_constants();
  sum_views();
  binary_payloads();
  word_descriptors();
  rec8();
  alldiff();
  formula_trees();
  big_tables();
  validators();
  std::printf("all ok\n");
  return 0;
}
