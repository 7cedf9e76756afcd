// pcp_lower.hip — model lowering (pcp_lower.h): the arithmetic between the pushed pcp_props and the tables the kernels read.
// Host code only and free of HIP: it also compiles as plain C++ (g++ -x c++), which is how tests/lower_check.cpp checks it.
#include "pcp_lower.h"

#include <algorithm>
#include <climits>
#include <cstring>
#include <map>
#include <utility>

namespace pcp {

namespace {

int32_t fail(std::string& err, int32_t code, const char* msg) {
  err = msg;
  return code;
}

int arity(uint8_t kind) { return kind >= PCP_BOOL ? 1 : (kind <= PCP_LT ? 2 : 3); }
bool is_sum_operand(uint32_t var) { return var >= PCP_SUM && var < PCP_NOVAR; }

// floor(log2(len)), len >= 1: the table level a slot range of that length is queried at
uint32_t range_level(uint32_t len) { uint32_t k = 0; while ((2u << k) <= len) ++k; return k; }

// Word and group descriptors for the level -1 test of packed tiles (WordDesc / GroupDesc, pcp_tables.h) over the P records of a compact model.
void lower_descriptors(const std::vector<Rec>& recs, size_t P, Lowered& out) {
  const size_t W = (P + 63) / 64;
  std::vector<WordDesc> wd(W + kStreamPadRecs / 64);
  size_t good = 0;
  bool any_lt = false;
  // one part: records [r0, r1) of one binary kind whose x and y slots each span < kRangeMax and whose offsets fit int16
  auto make_part = [&](size_t r0, size_t r1, WordPart& part) {
    const uint32_t kind = recs[r0].xk >> 28;
    if (kind != PCP_NEQ && kind != PCP_LT) return false;
    uint32_t xlo = ~0u, xhi = 0, ylo = ~0u, yhi = 0;
    int32_t dmin = INT32_MAX, dmax = INT32_MIN;
    for (size_t r = r0; r < r1; ++r) {
      if ((recs[r].xk >> 28) != kind) return false;
      const uint32_t x = recs[r].xk & kSlotMask, y = recs[r].y;
      xlo = std::min(xlo, x); xhi = std::max(xhi, x); ylo = std::min(ylo, y); yhi = std::max(yhi, y);
      dmin = std::min(dmin, recs[r].d); dmax = std::max(dmax, recs[r].d);
    }
    if (xhi - xlo >= kRangeMax || yhi - ylo >= kRangeMax || dmin < -30000 || dmax > 30000) return false;
    const uint32_t kx = range_level(xhi - xlo + 1), ky = range_level(yhi - ylo + 1);
    part.x = xlo | ((xhi - (1u << kx) + 1) << 16);
    part.y = ylo | ((yhi - (1u << ky) + 1) << 16);
    part.k = kx | (ky << 4) | ((kind == PCP_NEQ ? 1u : 2u) << 8);
    part.d = ((uint32_t)dmin & 0xffffu) | ((uint32_t)dmax << 16);
    any_lt |= kind == PCP_LT;
    return true;
  };
  for (size_t w = 0; w < W; ++w) {
    const size_t r0 = w * 64, r1 = std::min(P, r0 + 64);
    WordDesc q;
    memset(&q, 0, sizeof(q));
    if (make_part(r0, r1, q.a)) {
      ++good;
    } else {
      size_t rs = r0 + 1;  // first change of x
      while (rs < r1 && (recs[rs].xk & kSlotMask) == (recs[r0].xk & kSlotMask)) ++rs;
      WordPart pa, pb;
      if (rs < r1 && make_part(r0, rs, pa) && make_part(rs, r1, pb) && (pa.k >> 8) == (pb.k >> 8)) {
        q.a = pa; q.b = pb; q.a.k |= 1u << 12;
        ++good;
      } else {
        memset(&q, 0, sizeof(q));
      }
    }
    wd[w] = q;
  }
  if (!(W && good * 2 >= W && W <= 512u * 1024u)) return;  // worth a sweep organised by word groups (16-bit lane counters: <= 1023 groups per wavefront)
  out.wdesc = std::move(wd);
  out.word_level = any_lt ? 2 : 1;
  // group descriptors: the same idea one level up (64 words at a time; the y operands as a suffix [ylo, n_slots))
  const size_t G = (W + 63) / 64;
  out.gdesc.resize(G);
  for (size_t g = 0; g < G; ++g) {
    GroupDesc q;
    memset(&q, 0, sizeof(q));
    const size_t r0 = g * 4096, r1 = std::min(P, r0 + 4096);
    const uint32_t kind = recs[r0].xk >> 28;
    bool ok = kind == PCP_NEQ || kind == PCP_LT;
    uint32_t xlo = ~0u, xhi = 0, ylo = ~0u;
    int32_t dmin = INT32_MAX, dmax = INT32_MIN;
    for (size_t r = r0; r < r1 && ok; ++r) {
      ok = (recs[r].xk >> 28) == kind;
      const uint32_t x = recs[r].xk & kSlotMask;
      xlo = std::min(xlo, x); xhi = std::max(xhi, x); ylo = std::min(ylo, recs[r].y);
      dmin = std::min(dmin, recs[r].d); dmax = std::max(dmax, recs[r].d);
    }
    if (ok && xhi - xlo < kRangeMax && dmin >= -30000 && dmax <= 30000) {
      const uint32_t kx = range_level(xhi - xlo + 1);
      q.x = xlo | ((xhi - (1u << kx) + 1) << 16);
      q.k = kx | ((kind == PCP_NEQ ? 1u : 2u) << 8);
      q.ylo = ylo;
      q.d = ((uint32_t)dmin & 0xffffu) | ((uint32_t)dmax << 16);
    }
    out.gdesc[g] = q;
  }
}

// all-different units: every pair of a set of m <= 64 variables exactly once, as x != y without offsets
void lower_alldiff(const HostModel& m, const std::vector<Rec>& recs, size_t P, Lowered& out) {
  std::vector<uint32_t> tab{0u}, vars, mask((m.n_units + 31) / 32, 0u);
  size_t r = 0;
  while (r < P) {
    const uint32_t u = m.unit_of_prop[r];
    size_t e = r;
    while (e < P && m.unit_of_prop[e] == u) ++e;
    if (e - r >= 3 && m.props[r].group_kind != 0) {
      std::vector<uint32_t> vs;
      std::vector<std::pair<uint32_t, uint32_t>> pairs;
      bool ok = true;
      for (size_t k = r; k < e && ok; ++k) {
        const uint32_t x = recs[k].xk & kSlotMask, y = recs[k].y;
        ok = (recs[k].xk >> 28) == PCP_NEQ && recs[k].d == 0 && x < m.n_vars && y < m.n_vars && x != y;
        if (ok) { vs.push_back(x); vs.push_back(y); pairs.emplace_back(std::min(x, y), std::max(x, y)); }
      }
      if (ok) {
        std::sort(vs.begin(), vs.end()); vs.erase(std::unique(vs.begin(), vs.end()), vs.end());
        std::sort(pairs.begin(), pairs.end());
        const size_t n = vs.size();
        // (pcp_small.hip keeps the tables of up to 8 such units over up to 256 variables in LDS: kSmallAdUnits, kSmallAdVars)
        ok = n <= 64 && tab[0] < 8u && vars.size() + n <= 256 && pairs.size() == n * (n - 1) / 2 && std::adjacent_find(pairs.begin(), pairs.end()) == pairs.end();
        if (ok) {
          tab.push_back(u); tab.push_back((uint32_t)n); tab.push_back((uint32_t)vars.size());
          vars.insert(vars.end(), vs.begin(), vs.end());
          mask[u >> 5] |= 1u << (u & 31u);
          ++tab[0];
        }
      }
    }
    r = e;
  }
  if (!tab[0]) return;
  out.n_alldiff = tab[0];
  out.ad_tab = std::move(tab); out.ad_vars = std::move(vars); out.ad_mask = std::move(mask);
}

// every unit as a tree for pcp_formula.hip: a standalone propagator = one leaf, a Conjunction / Distinct group = an AND over
// its members, a formula = its own tree with the leaves renumbered to record indices
int32_t lower_formulas(const HostModel& m, size_t P, Lowered& out, std::string& err) {
  std::vector<pcp_fnode>& fn = out.fnodes;
  std::vector<uint32_t>& root = out.unit_root;
  root.assign(m.n_units + 1, 0);
  size_t r = 0;
  while (r < P) {
    const uint32_t u = m.unit_of_prop[r];
    size_t e = r;
    while (e < P && m.unit_of_prop[e] == u) ++e;
    root[u] = (uint32_t)fn.size();
    const int32_t f = m.formula_of_prop[r];
    if (f >= 0) {
      const auto& tree = m.formulas[(size_t)f];
      // (the kernel keeps a tree's node statuses in 64-bit masks; only a FLAT Conjunction of leaves may be wider — it is a loop)
      if (tree.size() > 64) {
        bool flat = tree[0].type == PCP_F_AND && (size_t)tree[0].n_children + 1 == tree.size();
        for (size_t i = 1; i < tree.size() && flat; ++i) flat = tree[i].type == PCP_F_LEAF;
        if (!flat) return fail(err, PCP_ERR_UNSUPPORTED, "a formula of more than 64 nodes (other than a flat Conjunction of propagators)");
      }
      const uint32_t base = (uint32_t)fn.size();
      for (const pcp_fnode& nd : tree) {
        pcp_fnode q = nd;
        q.first = nd.type == PCP_F_LEAF ? (uint32_t)r + nd.first : base + nd.first;
        fn.push_back(q);
      }
    } else if (e - r == 1) {
      fn.push_back(pcp_fnode{PCP_F_LEAF, 0, 0, (uint32_t)r});
    } else {
      if (e - r > 65535) return fail(err, PCP_ERR_UNSUPPORTED, "a Conjunction of more than 65535 members next to formula propagators");
      const uint32_t base = (uint32_t)fn.size();
      fn.push_back(pcp_fnode{PCP_F_AND, 0, (uint16_t)(e - r), base + 1});
      for (size_t k = r; k < e; ++k) fn.push_back(pcp_fnode{PCP_F_LEAF, 0, 0, (uint32_t)k});
    }
    r = e;
  }
  root[m.n_units] = (uint32_t)fn.size();  // (sentinel: a unit's nodes are root[u] .. root[u + 1])
  return PCP_OK;
}

}  // namespace

int32_t validate_prop(const HostModel& m, const pcp_prop& p, std::string& err) {
  if (p.kind > PCP_NBOOL) return fail(err, PCP_ERR_ARG, "unknown propagator kind");
  if (p.kind >= PCP_BOOL && m.set_words && !m.set_formulas) return fail(err, PCP_ERR_UNSUPPORTED, "the reified layer (Boolean / formulas) is interval mode only");
  if (p.group_kind > 2 || p.reserved != 0) return fail(err, PCP_ERR_ARG, "bad group_kind/reserved");
  const int n = arity(p.kind);
  std::vector<uint32_t> seen;  // every variable the propagator subscribes to, Sum members included
  for (int i = 0; i < n; ++i) {
    if (p.var[i] == PCP_NOVAR) return fail(err, PCP_ERR_ARG, "missing operand");
    if (p.off[i] > PCP_BOUND_MAX || p.off[i] < -PCP_BOUND_MAX) return fail(err, PCP_ERR_CONTRACT, "offset outside +-PCP_BOUND_MAX");
    if (p.var[i] == PCP_CONST) continue;
    if (is_sum_operand(p.var[i])) {
      const uint32_t t = p.var[i] & ~PCP_SUM;
      if (t >= m.sums.size()) return fail(err, PCP_ERR_ARG, "unknown Sum term (pcp_model_push_sum)");
      if (m.set_words) return fail(err, PCP_ERR_UNSUPPORTED, "Sum views over IntervalSet domains are not supported (interval mode only)");
      if (p.kind == PCP_MUL3) return fail(err, PCP_ERR_UNSUPPORTED, "XEqYMulZ over a Sum view is not supported");
      for (uint32_t v : m.sums[t]) seen.push_back(v);
      continue;
    }
    if (p.var[i] >= m.n_vars) return fail(err, PCP_ERR_CONTRACT, "variable index out of range (variable/store.rs:176-179)");
    seen.push_back(p.var[i]);
  }
  std::sort(seen.begin(), seen.end());
  if (std::adjacent_find(seen.begin(), seen.end()) != seen.end())
    return fail(err, PCP_ERR_CONTRACT, "propagator already subscribed to this variable (reactors/indexed_deps.rs:69-77)");
  if (p.kind == PCP_MUL3 && m.set_words)
    return fail(err, PCP_ERR_UNSUPPORTED, "XEqYMulZ over IntervalSet domains is not supported (interval mode only)");
  return PCP_OK;
}

int32_t validate_formula(const HostModel& m, uint32_t n_nodes, const pcp_fnode* nodes, uint32_t n_leaves, const pcp_prop* leaves, std::string& err) {
  if (m.set_words && !m.set_formulas) return fail(err, PCP_ERR_UNSUPPORTED, "formula propagators are interval mode only");
  std::vector<uint32_t> depth(n_nodes, 0), uses(n_nodes, 0), leaf_uses(n_leaves, 0);
  depth[0] = 1; uses[0] = 1;
  for (uint32_t i = 0; i < n_nodes; ++i) {
    const pcp_fnode& nd = nodes[i];
    if (nd.reserved != 0 || nd.type > PCP_F_OR) return fail(err, PCP_ERR_ARG, "bad formula node");
    if (uses[i] != 1) return fail(err, PCP_ERR_ARG, "formula node not reached exactly once from the root");
    if (depth[i] > 8) return fail(err, PCP_ERR_UNSUPPORTED, "formula deeper than 8 levels");
    if (nd.type == PCP_F_LEAF) {
      if (nd.first >= n_leaves) return fail(err, PCP_ERR_ARG, "formula leaf out of range");
      if (++leaf_uses[nd.first] != 1) return fail(err, PCP_ERR_ARG, "formula leaf used twice");
      continue;
    }
    if (nd.n_children == 0) return fail(err, PCP_ERR_CONTRACT, "a Conjunction / Disjunction needs at least one child");
    if (nd.first <= i || (uint64_t)nd.first + nd.n_children > n_nodes) return fail(err, PCP_ERR_ARG, "formula children out of range");
    for (uint32_t k = 0; k < nd.n_children; ++k) { ++uses[nd.first + k]; depth[nd.first + k] = depth[i] + 1; }
  }
  for (uint32_t i = 0; i < n_leaves; ++i) {
    if (leaf_uses[i] != 1) return fail(err, PCP_ERR_ARG, "formula leaf not used");
    int32_t rc = validate_prop(m, leaves[i], err);
    if (rc) return rc;
  }
  return PCP_OK;
}

int32_t lower_model(const HostModel& m, Lowered& out, std::string& err) {
  out = Lowered{};
  const size_t P = m.props.size();
  const uint32_t n_vars = m.n_vars;
  std::map<int32_t, uint32_t> const_slot;
  // slots: [0, n_vars) variables, [n_vars, n_vars + n_sum) Sum views of several members, then the interned constants.
  // `consts` covers every slot >= n_vars (the Sum slots hold 0: their domain is computed from the members on demand).
  std::vector<uint32_t> sum_slot(m.sums.size(), 0), sum_off(1, 0), sum_mem;
  uint32_t n_sum = 0;
  for (size_t t = 0; t < m.sums.size(); ++t) {
    if (m.sums[t].size() == 1) { sum_slot[t] = m.sums[t][0]; continue; }  // a Sum of one variable forwards to it (sum.rs:63-64)
    sum_slot[t] = n_vars + n_sum++;
    sum_mem.insert(sum_mem.end(), m.sums[t].begin(), m.sums[t].end());
    sum_off.push_back((uint32_t)sum_mem.size());
  }
  out.n_sum_slots = n_sum;
  std::vector<int32_t>& consts = out.consts;
  consts.assign(n_sum, 0);
  auto slot_of = [&](uint32_t var, int32_t value) -> uint32_t {
    if (is_sum_operand(var)) return sum_slot[var & ~PCP_SUM];
    if (var != PCP_CONST) return var;
    auto it = const_slot.find(value);
    if (it != const_slot.end()) return it->second;
    uint32_t s = n_vars + (uint32_t)consts.size();
    const_slot.emplace(value, s);
    consts.push_back(value);
    return s;
  };
  // every variable an operand makes the propagator depend on (ViewDependencies: identity.rs:66-69, sum.rs:85-91)
  auto for_each_dep = [&](uint32_t var, auto&& f) {
    if (var == PCP_CONST) return;
    if (is_sum_operand(var)) { for (uint32_t v : m.sums[var & ~PCP_SUM]) f(v); return; }
    f(var);
  };
  std::vector<Rec>& recs = out.recs;
  recs.assign(P, Rec{0, 0, 0, 0});
  std::vector<uint32_t> deg(n_vars + 1, 0);
  bool tern = false;
  for (size_t r = 0; r < P; ++r) {
    const pcp_prop& p = m.props[r];
    const int n = arity(p.kind);
    uint32_t s[3] = {0, 0, 0};
    int64_t off[3] = {0, 0, 0};
    for (int i = 0; i < n; ++i) {
      // a Constant operand carries its value in off[i]; as a pseudo-variable its offset is 0
      s[i] = slot_of(p.var[i], p.off[i]);
      off[i] = (p.var[i] == PCP_CONST) ? 0 : p.off[i];
    }
    int64_t d;
    if (n == 1) d = off[0];                       // Boolean / BooleanNeg over the view x + d
    else if (n == 2) d = off[1] - off[0];         // X = x, Y = y + d
    else if (p.kind == PCP_MUL3) {                // (x + dx) = (y + dy) * (z + dz): the offsets go to a side table, d = its index
      d = (int64_t)(out.mul_off.size() / 3);
      for (int i = 0; i < 3; ++i) out.mul_off.push_back((int32_t)off[i]);
    }
    else d = off[1] + off[2] - off[0];            // x  vs  y + z + d
    if (d > PCP_BOUND_MAX || d < -PCP_BOUND_MAX) return fail(err, PCP_ERR_CONTRACT, "folded offset outside +-PCP_BOUND_MAX");
    recs[r].xk = s[0] | ((uint32_t)p.kind << 28);
    recs[r].y = s[1];
    recs[r].z = (n == 3) ? s[2] : 0;
    recs[r].d = (int32_t)d;
    tern |= (n != 2);  // (Boolean leaves too: such stores take the formula kernel, never the binary fast paths)
    for (int i = 0; i < n; ++i) for_each_dep(p.var[i], [&](uint32_t v) { ++deg[v]; });
  }
  tern |= n_sum != 0;  // Sum views: generic path only (no compact stream, no adjacency payloads, no word descriptors)
  const uint32_t n_slots = n_vars + (uint32_t)consts.size();
  if (n_slots >= kMaxSlots) return fail(err, PCP_ERR_UNSUPPORTED, "too many variables");
  out.n_slots = n_slots;
  out.has_ternary = tern;
  if (n_sum) { out.sum_off = std::move(sum_off); out.sum_mem = std::move(sum_mem); }

  // CSR adjacency: variable -> the records that depend on it, in record order
  std::vector<uint32_t>& adj_off = out.adj_off;
  std::vector<uint32_t>& adj = out.adj;
  adj_off.assign(n_vars + 1, 0);
  for (uint32_t v = 0; v < n_vars; ++v) adj_off[v + 1] = adj_off[v] + deg[v];
  for (uint32_t v = 0; v < n_vars; ++v) out.max_deg = std::max(out.max_deg, deg[v]);
  adj.assign(adj_off[n_vars], 0);
  {
    std::vector<uint32_t> fill(adj_off.begin(), adj_off.end() - 1);
    for (size_t r = 0; r < P; ++r) {
      const pcp_prop& p = m.props[r];
      for (int i = 0; i < arity(p.kind); ++i) for_each_dep(p.var[i], [&](uint32_t v) { adj[fill[v]++] = (uint32_t)r; });
    }
  }
  const size_t Ppad = P ? ((P + 255) / 256) * 256 + kStreamPadRecs : 0;  // see kStreamPadRecs
  if (P) { const Rec last = recs[P - 1]; recs.resize(Ppad, last); }
  if (P && !n_sum) {
    const uint32_t k0 = recs[0].xk >> 28;
    bool same = (k0 == PCP_NEQ || k0 == PCP_LT);
    for (size_t r = 1; r < P && same; ++r) same = (recs[r].xk >> 28) == k0;
    if (same) out.uniform_kind = k0;
  }
  if (!tern && !adj.empty()) {  // adjacency payloads (ModelDev::adjp)
    out.adjp.resize(adj.size());
    std::vector<uint32_t> fill(adj_off.begin(), adj_off.end() - 1);
    for (size_t r = 0; r < P; ++r) {
      const uint32_t x = recs[r].xk & kSlotMask, y = recs[r].y, kind = recs[r].xk >> 28;
      if (x < n_vars) out.adjp[fill[x]++] = U32x2{y | (kind << 28), (uint32_t)recs[r].d};
      if (y < n_vars) out.adjp[fill[y]++] = U32x2{x | (kind << 28) | (1u << 31), (uint32_t)recs[r].d};
    }
    out.have_adjp = true;
  }
  // assignment-driven path (pcp_neq.hip): all-XNeqY models.  A record over two constants has no variable whose list would
  // run it: such (degenerate) models keep the generic kernels.  Variables with a Constant neighbour are walked in round 0
  // whatever their domain — the constant is a singleton without a list of its own.
  out.neq_model = out.uniform_kind == PCP_NEQ && out.have_adjp && n_slots < 65536u;
  if (out.neq_model) {
    std::vector<uint32_t> seed((n_slots + 31) / 32, 0u);
    bool any = false;
    for (size_t r = 0; r < P && out.neq_model; ++r) {
      const uint32_t x = recs[r].xk & kSlotMask, y = recs[r].y;
      if (x >= n_vars && y >= n_vars) out.neq_model = false;
      else if (x >= n_vars) { seed[y >> 5] |= 1u << (y & 31); any = true; }
      else if (y >= n_vars) { seed[x >> 5] |= 1u << (x & 31); any = true; }
    }
    if (out.neq_model && n_slots <= 32768u) {
      bool fits = true;
      for (size_t r = 0; r < P && fits; ++r) fits = recs[r].d >= -32767 && recs[r].d <= 32767;
      if (fits) {
        // (one zero entry behind the last list: the lean round 0 requests a listed variable's first entry whatever its degree — neq_fast_load —,
        // and for a last variable without records that is the entry at adj_off[n_vars])
        out.adjp4.assign(adj.size() + 1, 0u);
        std::vector<uint32_t> fill(adj_off.begin(), adj_off.end() - 1);
        for (size_t r = 0; r < P; ++r) {
          const uint32_t x = recs[r].xk & kSlotMask, y = recs[r].y;
          const int32_t d = recs[r].d;
          if (x < n_vars) out.adjp4[fill[x]++] = y | ((uint32_t)(uint16_t)(int16_t)(-d) << 16);
          if (y < n_vars) out.adjp4[fill[y]++] = x | (1u << 15) | ((uint32_t)(uint16_t)(int16_t)d << 16);
        }
        out.have_adjp4 = true;
      }
    }
    if (out.neq_model && any) {
      out.seed_always = std::move(seed);
      out.have_seed_always = true;
    }
  }
  out.compact = !tern && n_slots <= kCompactSlots && P > 0;
  for (int32_t v : consts) out.consts_fit16 &= (v >= -kPackedMax && v <= kPackedMax);
  if (out.compact) {
    out.recs8.resize(Ppad);
    for (size_t r = 0; r < Ppad; ++r) {
      out.recs8[r].xyk = (recs[r].xk & kSlotMask) | (recs[r].y << 15) | ((recs[r].xk >> 28) << 30);
      out.recs8[r].d = recs[r].d;
    }
    lower_descriptors(recs, P, out);
  }
  if (m.has_groups) {
    out.unit_first.assign(m.n_units + 1, (uint32_t)P);
    for (size_t r = P; r-- > 0;) out.unit_first[m.unit_of_prop[r]] = (uint32_t)r;
  }
  if (m.has_groups && !m.has_formulas) lower_alldiff(m, recs, P, out);
  if (m.has_formulas) return lower_formulas(m, P, out, err);
  return PCP_OK;
}

bool lower_big(const std::vector<Rec>& recs, const std::vector<uint32_t>& adj_off, const std::vector<uint32_t>& adj, const std::vector<int32_t>& consts,
               uint32_t n_vars, uint32_t n_recs, bool bank_order, std::vector<U32x2>& brec, std::vector<U32x2>& badj) {
  const size_t P = n_recs;
  const uint32_t nv = n_vars;
  if (nv >= 98304u) return false;
  // a record with a Constant operand becomes a unary record  var (op) K:  x (kind) c + d  /  c (kind) y + d  <=>  y (>, =, !=) c - d
  struct BR { U32x2 r; uint32_t key; };
  std::vector<BR> br(P);
  auto coord = [](uint32_t slot) { return (slot / 3u) | ((slot % 3u) << 15); };
  for (size_t r = 0; r < P; ++r) {
    const uint32_t x = recs[r].xk & kSlotMask, y = recs[r].y, kind = recs[r].xk >> 28;
    const int64_t d = recs[r].d;
    if (kind > PCP_LT || (x >= nv && y >= nv)) return false;
    // (the folded constant K is computed in 64 bits and must stay far inside int32: the kernel forms K - lo, K - 1 and K + 1; a model
    // whose constant and offset add up to more than 2^30 in magnitude goes to the generic kernels instead of being wrapped)
    constexpr int64_t kFoldMax = (int64_t)1 << 30;
    if (y >= nv) {         // x (kind) K,  K = c + d
      const uint32_t op = kind == PCP_LT ? 0u : kind == PCP_EQ ? 2u : 3u;
      const int64_t K = (int64_t)consts[y - nv] + d;
      if (K < -kFoldMax || K > kFoldMax) return false;
      br[r] = BR{U32x2{coord(x) | (op << 17) | (3u << 30), (uint32_t)(int32_t)K}, 3u};
    } else if (x >= nv) {  // c (kind) y + d:  LT  y > c - d  |  EQ  y = c - d  |  NEQ  y != c - d
      const uint32_t op = kind == PCP_LT ? 1u : kind == PCP_EQ ? 2u : 3u;
      const int64_t K = (int64_t)consts[x - nv] - d;
      if (K < -kFoldMax || K > kFoldMax) return false;
      br[r] = BR{U32x2{coord(y) | (op << 17) | (3u << 30), (uint32_t)(int32_t)K}, 3u};
    } else {
      if (d < -4095 || d > 4095) return false;
      br[r] = BR{U32x2{coord(x) | (((uint32_t)(int32_t)d & 0x1fffu) << 17) | (kind << 30), coord(y)}, kind};
    }
  }
  // the adjacency payloads first (they follow ModelDev::adj, which names records of the UNSORTED table)
  badj.assign(adj.size(), U32x2{0, 0});
  for (uint32_t v = 0; v < nv; ++v)
    for (uint32_t k = adj_off[v]; k < adj_off[v + 1]; ++k) {
      const Rec& rec = recs[adj[k]];
      const BR& b = br[adj[k]];
      const uint32_t x = rec.xk & kSlotMask, y = rec.y, kind = rec.xk >> 28;
      if (b.key == 3u) { badj[k] = U32x2{0x7fffu | (((b.r.x >> 17) & 3u) << 18) | (1u << 20), b.r.y}; continue; }
      const bool is_y = x != v;
      badj[k] = U32x2{coord(is_y ? x : y) | ((is_y ? 1u : 0u) << 17) | (kind << 18), (uint32_t)rec.d};
    }
  std::stable_sort(br.begin(), br.end(), [](const BR& p, const BR& q) { return p.key < q.key; });
  // Bank-aware order within a kind (the order of the table is free — every fair schedule reaches the same fixpoint, DESIGN.md §2 —
  // and the model is immutable).  A cell word is 8 bytes = one PAIR of LDS banks, and a wavefront's ds_read_b64 / 64-bit compare-and-swap is
  // served one 32-lane half at a time: it is conflict-free iff the half's 32 word indices differ mod 32.  With the model's own (random) order a
  // half hit ~12 distinct bank pairs out of 32 twice or more: SQ_LDS_BANK_CONFLICT was 0.44 of SQ_LDS_IDX_ACTIVE (profiles/r05_c3_*).  Greedy:
  // the records of a kind are dealt from 32 buckets (x word mod 32), one per lane of a half, preferring among a bucket's next few records one
  // whose y word falls on a bank pair the half has not used yet.  Neighbouring lanes then never compare-and-swap the same word either.
  if (bank_order) {
    size_t s0 = 0;
    while (s0 < P) {
      size_t e0 = s0;
      while (e0 < P && br[e0].key == br[s0].key) ++e0;
      std::vector<uint32_t> bucket[32];
      for (size_t r = s0; r < e0; ++r) bucket[br[r].r.x & 31u].push_back((uint32_t)r);
      size_t head[32] = {0};
      std::vector<BR> dealt;
      dealt.reserve(e0 - s0);
      const bool unary = br[s0].key == 3u;
      size_t pos = s0;           // table position of the next record: halves are positions [32 h, 32 h + 32)
      uint32_t usedx = 0, usedy = 0;
      uint32_t rot = 0;
      while (dealt.size() < e0 - s0) {
        if ((pos & 31u) == 0) { usedx = 0; usedy = 0; }
        // the fullest bucket whose bank pair this half has not used (ties: rotate), else the fullest bucket at all
        int best = -1; size_t best_n = 0;
        for (uint32_t i = 0; i < 32; ++i) {
          const uint32_t b = (i + rot) & 31u;
          const size_t n = bucket[b].size() - head[b];
          if (n > best_n && !((usedx >> b) & 1u)) { best_n = n; best = (int)b; }
        }
        if (best < 0)
          for (uint32_t b = 0; b < 32; ++b) { const size_t n = bucket[b].size() - head[b]; if (n > best_n) { best_n = n; best = (int)b; } }
        std::vector<uint32_t>& bk = bucket[best];
        size_t pick = head[best];
        if (!unary)
          for (size_t k2 = head[best]; k2 < std::min(bk.size(), head[best] + 16); ++k2)
            if (!((usedy >> (br[bk[k2]].r.y & 31u)) & 1u)) { pick = k2; break; }
        std::swap(bk[pick], bk[head[best]]);
        const BR& chosen = br[bk[head[best]++]];
        usedx |= 1u << (chosen.r.x & 31u);
        if (!unary) usedy |= 1u << (chosen.r.y & 31u);
        dealt.push_back(chosen);
        ++pos; ++rot;
      }
      std::copy(dealt.begin(), dealt.end(), br.begin() + s0);
      s0 = e0;
    }
  }
  const size_t Ppad = P ? (P + 255) / 256 * 256 + kStreamPadRecs : 0;
  brec.resize(Ppad);
  for (size_t r = 0; r < Ppad; ++r) brec[r] = br[std::min<size_t>(r, P - 1)].r;
  return true;
}

}  // namespace pcp
