// Rule preconditions: Go-exact condition evaluator, compile-time interning, per-batch truth
// tables (kvcond.h).
#include "kvcond.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "kvpre.h"
#include "kvdeny.h"
#include "kvforeach.h"

namespace kvh {

using namespace kv;

namespace {

std::string lower(std::string s) {
  for (char& c : s)
    if (c >= 'A' && c <= 'Z') c = (char)(c - 'A' + 'a');
  return s;
}

// float64 -> int64 conversion of amd64 (CVTTSD2SQ): out of range and NaN give the minimum
int64_t go_f2i(double f) {
  if (!(f >= -9223372036854775808.0 && f < 9223372036854775808.0)) return INT64_MIN;
  return (int64_t)f;
}

// Duration.Seconds() (time.go): sec + nsec / 1e9
double dur_seconds(int64_t d) {
  const int64_t sec = d / 1000000000ll, nsec = d % 1000000000ll;
  return (double)sec + (double)nsec / 1e9;
}

// parseDuration (operator.go:80-139): at least one operand is a duration string other than "0";
// the other one is then a duration string or a number of seconds
bool parse_durations(const PV& key, const PV& value, double* ks, double* vs) {
  int64_t kd = 0, vd = 0;
  const bool kok = key.t == J_STR && key.s != "0" && go_parse_duration(key.s, &kd);
  const bool vok = value.t == J_STR && value.s != "0" && go_parse_duration(value.s, &vd);
  if (!kok && !vok) return false;
  if (!kok) {
    if (key.t != J_FLOAT) return false;
    kd = (int64_t)((uint64_t)go_f2i(key.f) * 1000000000ull);  // time.Duration(f) * time.Second (wraps)
  }
  if (!vok) {
    if (value.t != J_FLOAT) return false;
    vd = (int64_t)((uint64_t)go_f2i(value.f) * 1000000000ull);
  }
  *ks = dur_seconds(kd);
  *vs = dur_seconds(vd);
  return true;
}

// Quantity.Cmp of two parsed quantities (the canonical form of gocompat.cpp)
int qcanon_cmp(const QCanon& a, const QCanon& b) {
  const int sa = a.zero ? 0 : (a.neg ? -1 : 1), sb = b.zero ? 0 : (b.neg ? -1 : 1);
  if (sa != sb) return sa < sb ? -1 : 1;
  if (sa == 0) return 0;
  int m = 0;
  if (a.exp != b.exp) m = a.exp < b.exp ? -1 : 1;
  else if (a.hi != b.hi) m = a.hi < b.hi ? -1 : 1;
  else if (a.lo != b.lo) m = a.lo < b.lo ? -1 : 1;
  return sa > 0 ? m : -m;
}

// compareByCondition (numeric.go:30-52)
bool cmp_by(uint32_t op, double k, double v) {
  switch (op) {
    case CD_GE: return k >= v;
    case CD_GT: return k > v;
    case CD_LE: return k <= v;
    case CD_LT: return k < v;
    default: return false;
  }
}

// EqualHandler / NotEqualHandler (equal.go, notequal.go): `ne` selects the NotEqual results
bool eval_equal(const PV& key, const PV& value, bool ne) {
  switch (key.t) {
    case J_BOOL:  // validateValueWithBoolPattern
      if (value.t != J_BOOL) return ne;
      return (key.b == value.b) != ne;
    case J_FLOAT:  // validateValueWithFloatPattern (a decoded number is never int / int64)
      if (value.t == J_FLOAT) return (value.f == key.f) != ne;
      if (value.t == J_STR) {
        double f;
        if (!go_parse_float(value.s, &f)) return ne;
        return (f == key.f) != ne;
      }
      return ne;
    case J_STR: {  // validateValueWithStringPattern: duration, quantity, wildcard
      double ks, vs;
      if (parse_durations(key, value, &ks, &vs)) return (ks == vs) != ne;
      const QCanon qk = parse_quantity(key.s);
      if (qk.valid && value.t == J_STR) {
        const QCanon qv = parse_quantity(value.s);
        if (!qv.valid) return false;  // (both handlers: "parse error", false)
        return (qcanon_cmp(qk, qv) == 0) != ne;
      }
      if (value.t == J_STR) return wildcard_match_host(value.s, key.s) != ne;
      return ne;
    }
    default:  // nil: "Unsupported type", false in both handlers
      return false;
  }
}

bool eval_numeric_float(uint32_t op, double key, const PV& value) {  // numeric.go:100-127
  if (value.t == J_FLOAT) return cmp_by(op, key, value.f);
  if (value.t == J_STR) {
    PV k;
    k.t = J_FLOAT;
    k.f = key;
    double ks, vs;
    if (parse_durations(k, value, &ks, &vs)) return cmp_by(op, ks, vs);
    double f;
    if (go_parse_float(value.s, &f)) return cmp_by(op, key, f);
    int64_t i;
    if (go_parse_int(value.s, &i)) return cmp_by(op, key, (double)i);
    return false;
  }
  return false;
}

bool eval_numeric(uint32_t op, const PV& key, const PV& value) {  // numeric.go:54-168
  if (key.t == J_FLOAT) return eval_numeric_float(op, key.f, value);
  if (key.t != J_STR) return false;
  double ks, vs;
  if (parse_durations(key, value, &ks, &vs)) return cmp_by(op, ks, vs);
  double f;
  if (go_parse_float(key.s, &f)) return eval_numeric_float(op, f, value);
  int64_t i;
  if (go_parse_int(key.s, &i)) {  // validateValueWithIntPattern: float64(key) against the value
    return eval_numeric_float(op, (double)i, value);
  }
  const QCanon qk = parse_quantity(key.s);
  if (qk.valid) {
    if (value.t != J_STR) return false;
    const QCanon qv = parse_quantity(value.s);
    if (!qv.valid) return false;
    return cmp_by(op, (double)qcanon_cmp(qk, qv), 0.0);
  }
  return false;
}

// fmt.Sprint of a scalar
bool sprint(const PV& v, std::string* out) {
  switch (v.t) {
    case J_NULL: *out = "<nil>"; return true;
    case J_BOOL: *out = v.b ? "true" : "false"; return true;
    case J_FLOAT: *out = go_format_g(v.f); return true;
    case J_STR: *out = v.s; return true;
    default: return false;
  }
}

// json.Unmarshal([]byte(s), &[]string): null is an empty list, a null element ""
bool json_string_array(const std::string& s, std::vector<std::string>* out) {
  JDoc d;
  try {
    parse_json(s.data(), s.size(), NUM_FLOAT, &d);
  } catch (const std::exception&) {
    return false;
  }
  const JNode& r = d.at(d.root);
  if (r.t == J_NULL) return true;
  if (r.t != J_ARR) return false;
  for (uint32_t c = r.first; c < r.first + r.count; c++) {
    const JNode& e = d.at(c);
    if (e.t == J_STR) out->push_back(std::string(d.sval(e)));
    else if (e.t == J_NULL) out->push_back("");
    else return false;
  }
  return true;
}

// keyExistsInArray (in.go:58-94): 0 no, 1 yes, -1 invalid type
int key_exists(const std::string& key, const PV& value, bool* range) {
  if (value.t == J_ARR) {
    for (const PV& e : value.a) {
      std::string s;
      if (!sprint(e, &s)) { *range = true; return -1; }
      if (wildcard_match_host(key, s)) return 1;
    }
    return 0;
  }
  if (value.t == J_STR) {
    if (wildcard_match_host(value.s, key)) return 1;
    std::vector<std::string> arr;
    if (!json_string_array(value.s, &arr)) return -1;
    for (const std::string& e : arr)
      if (e == key) return 1;
    return 0;
  }
  return -1;
}

}  // namespace

uint32_t cond_op(const std::string& name) {
  const std::string s = lower(name);
  if (s == "equal" || s == "equals") return CD_EQ;
  if (s == "notequal" || s == "notequals") return CD_NE;
  if (s == "in") return CD_IN;
  if (s == "anyin") return CD_ANYIN;
  if (s == "allin") return CD_ALLIN;
  if (s == "notin") return CD_NOTIN;
  if (s == "anynotin") return CD_ANYNOTIN;
  if (s == "allnotin") return CD_ALLNOTIN;
  if (s == "greaterthanorequals") return CD_GE;
  if (s == "greaterthan") return CD_GT;
  if (s == "lessthanorequals") return CD_LE;
  if (s == "lessthan") return CD_LT;
  if (s == "durationgreaterthanorequals" || s == "durationgreaterthan" || s == "durationlessthanorequals" ||
      s == "durationlessthan")
    return CD_DURATION;
  return CD_UNKNOWN;
}

// time.ParseDuration (format.go): [-+]?([0-9]*(\.[0-9]*)?[a-z]+)+, "0" alone is zero
bool go_parse_duration(const std::string& str, int64_t* out) {
  size_t i = 0;
  const size_t n = str.size();
  bool neg = false;
  if (n && (str[0] == '-' || str[0] == '+')) {
    neg = str[0] == '-';
    i = 1;
  }
  if (str.compare(i, std::string::npos, "0") == 0) { *out = 0; return true; }
  if (i == n) return false;
  const uint64_t lim = 1ull << 63;
  uint64_t d = 0;
  auto digit = [&](size_t k) { return k < n && str[k] >= '0' && str[k] <= '9'; };
  while (i < n) {
    uint64_t v = 0, f = 0;
    double scale = 1.0;
    if (!(str[i] == '.' || digit(i))) return false;
    const size_t p0 = i;
    while (digit(i)) {  // leadingInt
      if (v > lim / 10) return false;
      v = v * 10 + (uint64_t)(str[i] - '0');
      if (v > lim) return false;
      i++;
    }
    const bool pre = i != p0;
    bool post = false;
    if (i < n && str[i] == '.') {
      i++;
      const size_t p1 = i;
      bool overflow = false;
      while (digit(i)) {  // leadingFraction
        if (!overflow) {
          if (f > (lim - 1) / 10) overflow = true;
          else {
            const uint64_t y = f * 10 + (uint64_t)(str[i] - '0');
            if (y > lim) overflow = true;
            else { f = y; scale *= 10; }
          }
        }
        i++;
      }
      post = i != p1;
    }
    if (!pre && !post) return false;
    const size_t u0 = i;
    while (i < n && str[i] != '.' && !digit(i)) i++;
    if (i == u0) return false;
    const std::string u = str.substr(u0, i - u0);
    uint64_t unit;
    if (u == "ns") unit = 1;
    else if (u == "us" || u == "\xC2\xB5s" || u == "\xCE\xBCs") unit = 1000;
    else if (u == "ms") unit = 1000000;
    else if (u == "s") unit = 1000000000ull;
    else if (u == "m") unit = 60ull * 1000000000ull;
    else if (u == "h") unit = 3600ull * 1000000000ull;
    else return false;
    if (v > lim / unit) return false;
    v *= unit;
    if (f > 0) {
      v += (uint64_t)((double)f * ((double)unit / scale));
      if (v > lim) return false;
    }
    d += v;
    if (d > lim) return false;
  }
  if (neg) { *out = (int64_t)(0 - d); return true; }
  if (d > lim - 1) return false;
  *out = (int64_t)d;
  return true;
}

bool cond_eval(uint32_t op, const PV& key, const PV& value, bool* range) {
  *range = false;
  if (op == CD_DURATION || key.t == J_MAP || key.t == J_ARR || value.t == J_MAP) {
    *range = true;
    return false;
  }
  if (value.t == J_ARR)
    for (const PV& e : value.a)
      if (e.t == J_MAP || e.t == J_ARR) { *range = true; return false; }
  switch (op) {
    case CD_EQ: return eval_equal(key, value, false);
    case CD_NE: return eval_equal(key, value, true);
    case CD_GT:
    case CD_GE:
    case CD_LT:
    case CD_LE: return eval_numeric(op, key, value);
    case CD_IN:
    case CD_ANYIN:
    case CD_ALLIN:
    case CD_NOTIN:
    case CD_ANYNOTIN:
    case CD_ALLNOTIN: {
      // scalar keys (in.go:30-46 and its siblings): a string, or fmt.Sprint of a number; every
      // other key type is "Unsupported type", false
      std::string k;
      if (key.t == J_STR) k = key.s;
      else if (key.t == J_FLOAT) k = go_format_g(key.f);
      else return false;
      const int e = key_exists(k, value, range);
      if (e < 0) return false;  // invalid type: false in every handler
      const bool notin = op == CD_NOTIN || op == CD_ANYNOTIN || op == CD_ALLNOTIN;
      return notin ? e == 0 : e == 1;
    }
    default: return false;  // unknown operator: CreateOperatorHandler returns nil (evaluate.go:13-16)
  }
}

// ------------------------------------------------------------------ compile
namespace {

bool has_escape_or_ref(const std::string& s) {
  return s.find("$(") != std::string::npos || s.find("\\{{") != std::string::npos;
}

bool tree_has_var(const PV& p) {
  if (p.t == J_STR) return var_string(p.s) || has_escape_or_ref(p.s);
  for (const PV& e : p.a)
    if (tree_has_var(e)) return true;
  for (size_t i = 0; i < p.mv.size(); i++)
    if (tree_has_var(p.mv[i]) || var_string(p.mk[i]) || has_escape_or_ref(p.mk[i])) return true;
  return false;
}

// a constant operand: a scalar or a list of scalars
bool const_operand_ok(const PV& p, bool is_key) {
  if (p.t == J_MAP) return false;
  if (p.t == J_ARR) {
    if (is_key) return false;  // (list keys: the set forms of the In family stay on the CPU route)
    for (const PV& e : p.a)
      if (e.t == J_MAP || e.t == J_ARR) return false;
  }
  return true;
}

std::string pv_key(const PV& p) {  // interning key of a constant operand
  switch (p.t) {
    case J_NULL: return "n";
    case J_BOOL: return p.b ? "b1" : "b0";
    case J_FLOAT: { std::string o = "f"; o.append((const char*)&p.f, 8); return o; }
    case J_STR: return "s" + std::to_string(p.s.size()) + ":" + p.s;
    default: {
      std::string o = "[";
      for (const PV& e : p.a) o += pv_key(e) + ",";
      return o + "]";
    }
  }
}

// The interning tables a block compiles into: the preconditions' (PolicySet::ckeys / conds) or
// the deny blocks' (dkeys / dconds). strs (deny): every condition string of the block, those of
// conditions folded to a constant included.
struct CondSpace {
  std::vector<std::string>& keys;
  std::vector<CondRec>& conds;
  std::unordered_map<std::string, uint32_t>& key_id;
  std::unordered_map<std::string, uint32_t>& cond_id;
  std::vector<uint32_t>* strs;
  size_t any_strs = 0;  // how many of them the `any` list gave (it is compiled first)
  // foreach entries: `element` is a variable root too, and the strings are interned under
  // tag + text (the list and the resolver mode: PolicySet::ftags)
  bool element = false;
  std::string tag;
};

// one condition: 0 constant false, 1 constant true, 2 dynamic (*rec), -1 outside the scope
int compile_condition(CondSpace& sp, const JDoc& d, uint32_t node, uint32_t* rec) {
  if (d.at(node).t != J_MAP) return -1;
  const int64_t kn = d.get(node, "key"), on = d.get(node, "operator"), vn = d.get(node, "value");
  if (kn < 0 || vn < 0) return -1;
  const JNode& cn = d.at(node);
  for (uint32_t c = cn.first; c < cn.first + cn.count; c++) {
    const std::string_view k = d.key(d.at(c));
    if (k != "key" && k != "operator" && k != "value") return -1;
  }
  std::string opname;
  if (on >= 0) {
    if (d.at((uint32_t)on).t != J_STR) return -1;
    opname = std::string(d.sval(d.at((uint32_t)on)));
    if (var_string(opname) || has_escape_or_ref(opname)) return -1;
  }
  const uint32_t op = cond_op(opname);
  if (op == CD_DURATION) return -1;
  const PV key = to_pv(d, (uint32_t)kn), value = to_pv(d, (uint32_t)vn);
  const bool kv = key.t == J_STR && var_string(key.s), vv = value.t == J_STR && var_string(value.s);
  if (kv && vv) return -1;
  for (const PV* p : {&key, &value}) {
    if (p->t == J_STR) {
      if (has_escape_or_ref(p->s)) return -1;
      if (var_string(p->s) && !cond_string_in_scope(p->s, sp.element)) return -1;
    } else if (tree_has_var(*p)) {
      return -1;  // variables inside a list or map operand
    }
  }
  if (!(kv ? true : const_operand_ok(key, true)) || !(vv ? true : const_operand_ok(value, false))) return -1;
  if (!kv && !vv) {  // folded
    bool range = false;
    const bool r = cond_eval(op, key, value, &range);
    return range ? -1 : (r ? 1 : 0);
  }
  if (op == CD_UNKNOWN && !sp.strs) return 0;
  const std::string text = sp.tag + (kv ? key.s : value.s);
  auto ck = sp.key_id.find(text);
  if (ck == sp.key_id.end()) {
    ck = sp.key_id.emplace(text, (uint32_t)sp.keys.size()).first;
    sp.keys.push_back(text);
  }
  if (sp.strs) sp.strs->push_back(ck->second);
  if (op == CD_UNKNOWN) return 0;  // (deny: the string still has to resolve)
  CondRec c;
  c.op = op;
  c.var_is_key = kv;
  c.cstr = ck->second;
  c.other = kv ? value : key;
  const std::string id = std::to_string(op) + (kv ? "k" : "v") + std::to_string(c.cstr) + "|" + pv_key(c.other);
  auto it = sp.cond_id.find(id);
  if (it == sp.cond_id.end()) {
    it = sp.cond_id.emplace(id, (uint32_t)sp.conds.size()).first;
    sp.conds.push_back(std::move(c));
  }
  *rec = it->second;
  return 2;
}

// An any / all block or the old list (utils.go:392-406 transformConditions, util.go:220-262)
// into *out, constants folded. False when the block is outside the device scope (the interning
// tables are left as they were); *always: no condition is left and none is a constant false.
bool compile_block(CondSpace& sp, const JDoc& d, uint32_t node, CondSet* out, bool* always) {
  const JNode& n = d.at(node);
  int64_t any = -1, all = -1;
  bool old_form = false;
  if (n.t == J_ARR) {
    old_form = true;  // []kyverno.Condition: AND (evaluate.go:69-78)
  } else if (n.t == J_MAP) {
    for (uint32_t c = n.first; c < n.first + n.count; c++) {
      const std::string_view k = d.key(d.at(c));
      if (k == "any") any = c;
      else if (k == "all") all = c;
      else return false;  // "unknown field" (util.go:223-239)
    }
  } else {
    return false;
  }
  // checkpoint of the interning tables: a block outside the scope leaves nothing behind
  const size_t ck0 = sp.keys.size(), cd0 = sp.conds.size();
  auto rollback = [&]() {
    for (size_t i = ck0; i < sp.keys.size(); i++) sp.key_id.erase(sp.keys[i]);
    sp.keys.resize(ck0);
    for (auto it = sp.cond_id.begin(); it != sp.cond_id.end();)
      it = it->second >= cd0 ? sp.cond_id.erase(it) : std::next(it);
    sp.conds.resize(cd0);
    if (sp.strs) sp.strs->clear();
    return false;
  };
  CondSet& s = *out;
  s = CondSet();
  bool any_true = false;
  auto list = [&](int64_t ln, bool is_any) {
    const JNode& l = d.at((uint32_t)ln);
    if (l.t != J_ARR) return false;
    for (uint32_t c = l.first; c < l.first + l.count; c++) {
      uint32_t rec = 0;
      const int r = compile_condition(sp, d, c, &rec);
      if (r < 0) return false;
      if (is_any) {
        if (r == 1) any_true = true;
        else if (r == 2) s.any.push_back(rec);
      } else {
        if (r == 0) s.const_false = true;
        else if (r == 2) s.all.push_back(rec);
      }
    }
    return true;
  };
  if (old_form) {
    if (!list(node, false)) return rollback();
  } else {
    if (any >= 0) {
      const JNode& l = d.at((uint32_t)any);
      if (l.t == J_NULL) any = -1;  // a nil list: absent
      else if (l.t != J_ARR || l.count == 0) return rollback();  // `any: []`: nil or empty after DeepCopy
    }
    if (all >= 0 && d.at((uint32_t)all).t == J_NULL) all = -1;
    if (any >= 0) {
      if (!list(any, true)) return rollback();
      if (sp.strs) sp.any_strs = sp.strs->size();
      if (any_true) s.any.clear();
      else {
        s.any_present = true;
        if (s.any.empty()) s.const_false = true;  // every member a constant false
      }
    }
    if (all >= 0 && !list(all, false)) return rollback();
  }
  if (s.const_false) {
    s.any.clear();
    s.all.clear();
    s.any_present = false;
  }
  *always = !s.const_false && !s.any_present && s.all.empty();
  // a lane loads each condition string once: its conditions follow each other
  auto by_str = [&](uint32_t a, uint32_t b) {
    return sp.conds[a].cstr != sp.conds[b].cstr ? sp.conds[a].cstr < sp.conds[b].cstr : a < b;
  };
  std::sort(s.any.begin(), s.any.end(), by_str);
  std::sort(s.all.begin(), s.all.end(), by_str);
  s.any.erase(std::unique(s.any.begin(), s.any.end()), s.any.end());
  s.all.erase(std::unique(s.all.begin(), s.all.end()), s.all.end());
  return true;
}

std::string set_key(const CondSet& s) {  // interning key of a folded block
  std::string id = s.const_false ? "F" : (s.any_present ? "A" : "-");
  for (uint32_t c : s.any) id += std::to_string(c) + ",";
  id += "|";
  for (uint32_t c : s.all) id += std::to_string(c) + ",";
  return id;
}

}  // namespace

uint32_t compile_preconditions(PolicySet& ps, const JDoc& d, uint32_t node) {
  CondSpace sp{ps.ckeys, ps.conds, ps.ckey_id, ps.cond_id, nullptr};
  CondSet s;
  bool always = false;
  if (!compile_block(sp, d, node, &s, &always)) return 0;
  if (always) return 0xFFFFFFFFu;
  const std::string id = set_key(s);
  auto it = ps.cset_id.find(id);
  if (it == ps.cset_id.end()) {
    it = ps.cset_id.emplace(id, (uint32_t)ps.csets.size()).first;
    ps.csets.push_back(std::move(s));
  }
  return it->second + 1;
}

uint32_t compile_deny(PolicySet& ps, const JDoc& d, uint32_t node) {
  // validate.deny: {conditions: <any / all block | old list>} (kyverno.Deny); `deny: {}` and a
  // missing or null `conditions` stay on the CPU route
  if (d.at(node).t != J_MAP) return 0;
  const JNode& n = d.at(node);
  int64_t cn = -1;
  for (uint32_t c = n.first; c < n.first + n.count; c++) {
    if (d.key(d.at(c)) != "conditions") return 0;
    cn = c;
  }
  if (cn < 0 || d.at((uint32_t)cn).t == J_NULL) return 0;
  DenySet s;
  CondSpace sp{ps.dkeys, ps.dconds, ps.dkey_id, ps.dcond_id, &s.strs};
  bool always = false;
  if (!compile_block(sp, d, (uint32_t)cn, &s.fold, &always)) return 0;
  // the strings in the order of the substitution's traversal with canonical key order, as for
  // pattern strings (kvvars.cpp): `all` before `any`, each list by index
  for (size_t i = sp.any_strs; i < s.strs.size(); i++) s.order.push_back(s.strs[i]);
  for (size_t i = 0; i < sp.any_strs; i++) s.order.push_back(s.strs[i]);
  std::sort(s.strs.begin(), s.strs.end());
  s.strs.erase(std::unique(s.strs.begin(), s.strs.end()), s.strs.end());
  std::string id = set_key(s.fold) + "#";
  for (uint32_t k : s.order) id += std::to_string(k) + ",";
  auto it = ps.dset_id.find(id);
  if (it == ps.dset_id.end()) {
    it = ps.dset_id.emplace(id, (uint32_t)ps.dsets.size()).first;
    ps.dsets.push_back(std::move(s));
  }
  return it->second + 1;
}

uint32_t compile_foreach(PolicySet& ps, const JDoc& d, uint32_t node) {
  // validate.foreach: a list of exactly one entry {list, preconditions?, deny} (with several, keys
  // of entry k-1's last element leak into entry k's `element`: kvcond.h)
  if (d.at(node).t != J_ARR || d.at(node).count != 1) return 0;
  const uint32_t en = d.at(node).first;
  if (d.at(en).t != J_MAP) return 0;
  int64_t ln = -1, pn = -1, dn = -1;
  for (uint32_t c = d.at(en).first; c < d.at(en).first + d.at(en).count; c++) {
    const std::string_view k = d.key(d.at(c));
    if (k == "list") ln = c;
    else if (k == "preconditions") pn = c;
    else if (k == "deny") dn = c;
    else return 0;  // pattern, anyPattern, context, ...
  }
  if (ln < 0 || dn < 0 || d.at((uint32_t)ln).t != J_STR || d.at((uint32_t)dn).t != J_MAP) return 0;
  const std::string list(d.sval(d.at((uint32_t)ln)));
  if (!list_query_in_scope(list)) return 0;
  if (pn >= 0 && d.at((uint32_t)pn).t == J_NULL) pn = -1;
  // the old list form of an entry's preconditions fails common.ToMap and is dropped by the
  // reference (validation.go:260-266): left to it
  if (pn >= 0 && d.at((uint32_t)pn).t != J_MAP) return 0;
  int64_t cn = -1;
  for (uint32_t c = d.at((uint32_t)dn).first; c < d.at((uint32_t)dn).first + d.at((uint32_t)dn).count; c++) {
    if (d.key(d.at(c)) != "conditions") return 0;
    cn = c;
  }
  if (cn < 0 || d.at((uint32_t)cn).t == J_NULL) return 0;
  // checkpoint: an entry outside the scope leaves nothing behind
  const size_t l0 = ps.flists.size(), k0 = ps.ftags.size(), c0 = ps.fconds.size();
  auto rollback = [&]() {
    for (size_t i = k0; i < ps.ftags.size(); i++) ps.ftag_id.erase(ps.ftags[i]);
    ps.ftags.resize(k0);
    for (auto it = ps.fcond_id.begin(); it != ps.fcond_id.end();)
      it = it->second >= c0 ? ps.fcond_id.erase(it) : std::next(it);
    ps.fconds.resize(c0);
    if (ps.flists.size() > l0) {
      ps.flist_id.erase(ps.flists.back());
      ps.flists.pop_back();
      ps.flist_keys.pop_back();
    }
    return 0u;
  };
  auto li = ps.flist_id.find(list);
  if (li == ps.flist_id.end()) {
    li = ps.flist_id.emplace(list, (uint32_t)ps.flists.size()).first;
    ps.flists.push_back(list);
    ps.flist_keys.emplace_back();
  }
  FeSet s;
  s.list = li->second;
  bool always = false;
  if (pn >= 0) {
    CondSpace sp{ps.ftags, ps.fconds, ps.ftag_id, ps.fcond_id, nullptr};
    sp.element = true;
    sp.tag = "p" + std::to_string(s.list) + ":";
    if (!compile_block(sp, d, (uint32_t)pn, &s.pre, &always)) return rollback();
    s.has_pre = !always;
    if (always) s.pre = CondSet();
  }
  CondSpace sp{ps.ftags, ps.fconds, ps.ftag_id, ps.fcond_id, &s.deny.strs};
  sp.element = true;
  sp.tag = "d" + std::to_string(s.list) + ":";
  if (!compile_block(sp, d, (uint32_t)cn, &s.deny.fold, &always)) return rollback();
  for (size_t i = sp.any_strs; i < s.deny.strs.size(); i++) s.deny.order.push_back(s.deny.strs[i]);
  for (size_t i = 0; i < sp.any_strs; i++) s.deny.order.push_back(s.deny.strs[i]);
  std::sort(s.deny.strs.begin(), s.deny.strs.end());
  s.deny.strs.erase(std::unique(s.deny.strs.begin(), s.deny.strs.end()), s.deny.strs.end());
  // the strings this entry added: their list, resolver mode and column in the list's element rows
  for (size_t i = ps.fkeys.size(); i < ps.ftags.size(); i++) {
    const std::string& t = ps.ftags[i];
    FeKey k;
    k.list = s.list;
    k.precond = t[0] == 'p';
    k.text = t.substr(t.find(':') + 1);
    k.col = (uint32_t)ps.flist_keys[s.list].size();
    ps.flist_keys[s.list].push_back((uint32_t)i);
    ps.fkeys.push_back(std::move(k));
  }
  std::string id = std::to_string(s.list) + "|" + (s.has_pre ? set_key(s.pre) : std::string("none")) + "|" +
                   set_key(s.deny.fold) + "#";
  for (uint32_t k : s.deny.order) id += std::to_string(k) + ",";
  auto it = ps.fset_id.find(id);
  if (it == ps.fset_id.end()) {
    it = ps.fset_id.emplace(id, (uint32_t)ps.fsets.size()).first;
    ps.fsets.push_back(std::move(s));
  }
  return it->second + 1;
}

// ------------------------------------------------------------------ per batch
namespace {

// Outcome ids per [condition string][res] of the C condition strings at column k0 of the
// outcome rows, and per condition the truth / unknown planes over the outcomes its string takes
// in this batch. err / oos (deny): per string, the outcomes that are a substitution error /
// outside the device scope.
void fill_planes(const PolicySet& ps, const Batch& b, const std::vector<CondRec>& conds, size_t k0, size_t C,
                 std::vector<uint32_t>* outc, std::vector<uint32_t>* truth, std::vector<uint32_t>* unk, uint32_t* words,
                 std::vector<uint32_t>* err, std::vector<uint32_t>* oos, const char* who) {
  const uint64_t n = b.res.size();
  const size_t K = ps.vout_width();
  // outcome ids, [condition string][res] (a lane's load is coalesced)
  outc->resize(C * n);
  if (b.vout.size() != K * n) throw std::runtime_error(std::string(who) + ": outcome rows do not match the policy set");
  for (uint64_t r = 0; r < n; r++)
    for (size_t c = 0; c < C; c++) (*outc)[c * n + r] = b.vout[r * K + k0 + c];
  // the outcomes each condition string takes in this batch
  const size_t T = b.vout_tab.size();
  const uint32_t W = (uint32_t)std::max<size_t>((T + 31) / 32, 1);
  *words = W;
  std::vector<uint32_t> seen(C * W, 0);
  for (size_t c = 0; c < C; c++)
    for (uint64_t r = 0; r < n; r++) {
      const uint32_t o = (*outc)[c * n + r];
      seen[c * W + o / 32] |= 1u << (o % 32);
    }
  if (err) {
    err->assign(C * W, 0);
    oos->assign(C * W, 0);
    for (size_t c = 0; c < C; c++)
      for (size_t o = 0; o < T; o++) {
        if (!((seen[c * W + o / 32] >> (o % 32)) & 1u)) continue;
        const char t = b.vout_tab[o].empty() ? 'C' : b.vout_tab[o][0];
        if (t == 'E') (*err)[c * W + o / 32] |= 1u << (o % 32);
        else if (!(t == 'S' || t == 'F' || t == 'B' || t == 'N' || t == 'M')) (*oos)[c * W + o / 32] |= 1u << (o % 32);
      }
  }
  truth->assign(conds.size() * W, 0);
  unk->assign(conds.size() * W, 0);
  for (size_t ci = 0; ci < conds.size(); ci++) {
    const CondRec& c = conds[ci];
    for (size_t o = 0; o < T; o++) {
      if (!((seen[c.cstr * W + o / 32] >> (o % 32)) & 1u)) continue;
      const std::string& oc = b.vout_tab[o];
      const char t = oc.empty() ? 'C' : oc[0];
      if (!(t == 'S' || t == 'F' || t == 'B' || t == 'N')) {  // a map / array, outside the scope
        (*unk)[ci * W + o / 32] |= 1u << (o % 32);
        continue;
      }
      const PV v = outcome_value(oc);
      bool range = false;
      const bool r = c.var_is_key ? cond_eval(c.op, v, c.other, &range) : cond_eval(c.op, c.other, v, &range);
      if (range) (*unk)[ci * W + o / 32] |= 1u << (o % 32);
      else if (r) (*truth)[ci * W + o / 32] |= 1u << (o % 32);
    }
  }
}

}  // namespace

void build_pre(const PolicySet& ps, const Batch& b, PreHost* out) {
  PreHost& h = *out;
  h = PreHost();
  if (ps.csets.empty()) return;
  const size_t k0 = ps.vkeys.size(), C = ps.ckeys.size();
  for (const CondSet& s : ps.csets) {
    h.sets.push_back((uint32_t)(h.ents.size() / 2));
    h.sets.push_back((uint32_t)s.any.size() | (s.any_present ? 0x80000000u : 0u));
    h.sets.push_back((uint32_t)s.all.size());
    h.sets.push_back(s.const_false ? 1u : 0u);
    for (uint32_t c : s.any) { h.ents.push_back(ps.conds[c].cstr); h.ents.push_back(c); }
    for (uint32_t c : s.all) { h.ents.push_back(ps.conds[c].cstr); h.ents.push_back(c); }
  }
  fill_planes(ps, b, ps.conds, k0, C, &h.outc, &h.truth, &h.unk, &h.words, nullptr, nullptr, "build_pre");
}

void build_deny(const PolicySet& ps, const Batch& b, DenyHost* out) {
  DenyHost& h = *out;
  h = DenyHost();
  if (ps.dsets.empty()) return;
  for (const DenySet& s : ps.dsets) {
    h.sets.push_back((uint32_t)(h.ents.size() / 2));
    const size_t e0 = h.ents.size();
    // one run of entries per string of the block, in string order: its `any` conditions, its
    // `all` conditions, or a bare entry where no condition of the string is left to evaluate
    for (uint32_t k : s.strs) {
      const size_t e1 = h.ents.size();
      for (uint32_t c : s.fold.any)
        if (ps.dconds[c].cstr == k) { h.ents.push_back(k); h.ents.push_back(c); }
      for (uint32_t c : s.fold.all)
        if (ps.dconds[c].cstr == k) { h.ents.push_back(k); h.ents.push_back(c | KV_DENY_ALL); }
      if (h.ents.size() == e1) { h.ents.push_back(k); h.ents.push_back(KV_DENY_NOCOND); }
    }
    h.sets.push_back((uint32_t)((h.ents.size() - e0) / 2));
    h.sets.push_back(s.fold.any_present ? 1u : 0u);
    h.sets.push_back(s.fold.const_false ? 1u : 0u);
  }
  fill_planes(ps, b, ps.dconds, ps.vkeys.size() + ps.ckeys.size(), ps.dkeys.size(), &h.outc, &h.truth, &h.unk, &h.words,
              &h.err, &h.oos, "build_deny");
}

uint8_t pre_status_host(const PreHost& h, uint32_t set, uint64_t n_res, uint64_t r) {
  return (uint8_t)kv_pre_lane(h.sets.data(), h.ents.data(), h.outc.data(), h.truth.data(), h.unk.data(), h.words, set,
                              n_res, r);
}

uint8_t deny_status_host(const DenyHost& h, uint32_t set, uint64_t n_res, uint64_t r) {
  return (uint8_t)kv_deny_lane(h.sets.data(), h.ents.data(), h.outc.data(), h.truth.data(), h.unk.data(), h.err.data(),
                               h.oos.data(), h.words, set, n_res, r);
}

// ------------------------------------------------------------------ foreach
void build_foreach(const PolicySet& ps, const Batch& b, FeHost* out) {
  FeHost& h = *out;
  h = FeHost();
  const uint64_t n = b.res.size();
  if (ps.fsets.empty() || n == 0) return;
  const size_t L = ps.flists.size();
  if (b.fstate.size() != L * n || b.fcount.size() != L * n || b.fout.size() != L)
    throw std::runtime_error("build_foreach: element rows do not match the policy set");
  // per list: the element blocks, [string][element] outcome ids, the per-resource state
  h.lstate.resize(L * n);
  h.first.resize(L * n);
  std::vector<uint32_t> plane0(L, 0);
  uint32_t rows = 0;
  for (size_t l = 0; l < L; l++) {
    const size_t K = ps.flist_keys[l].size();
    const uint32_t el0 = (uint32_t)h.el_res.size();
    for (uint64_t r = 0; r < n; r++) {
      h.lstate[l * n + r] = b.fstate[r * L + l];
      h.first[l * n + r] = (uint32_t)h.el_res.size() - el0;
      for (uint32_t i = 0; i < b.fcount[r * L + l]; i++) {
        h.el_res.push_back((uint32_t)r);
        h.el_ord.push_back(i);
      }
    }
    const uint32_t n_el = (uint32_t)h.el_res.size() - el0;
    if (b.fout[l].size() != (size_t)n_el * K) throw std::runtime_error("build_foreach: element rows misaligned");
    const uint32_t o0 = (uint32_t)h.outc.size();
    h.outc.resize(o0 + (size_t)n_el * K);
    for (uint32_t e = 0; e < n_el; e++)
      for (size_t c = 0; c < K; c++) h.outc[o0 + c * n_el + e] = b.fout[l][(size_t)e * K + c];
    plane0[l] = rows;
    h.lists.insert(h.lists.end(), {o0, n_el, rows, el0});
    rows += (uint32_t)K;
    h.max_el = std::max(h.max_el, n_el);
  }
  // the outcomes each string takes in this batch, then the planes over them
  const size_t T = b.vout_tab.size();
  const uint32_t W = (uint32_t)std::max<size_t>((T + 31) / 32, 1);
  h.words = W;
  std::vector<uint32_t> seen((size_t)rows * W, 0);
  auto row_of = [&](uint32_t key) { return plane0[ps.fkeys[key].list] + ps.fkeys[key].col; };
  for (size_t l = 0; l < L; l++) {
    const uint32_t o0 = h.lists[4 * l], n_el = h.lists[4 * l + 1];
    for (size_t c = 0; c < ps.flist_keys[l].size(); c++)
      for (uint32_t e = 0; e < n_el; e++) {
        const uint32_t o = h.outc[o0 + c * n_el + e];
        seen[(size_t)(plane0[l] + c) * W + o / 32] |= 1u << (o % 32);
      }
  }
  h.err.assign((size_t)rows * W, 0);
  h.oos.assign((size_t)rows * W, 0);
  for (size_t k = 0; k < ps.fkeys.size(); k++) {
    if (ps.fkeys[k].precond) continue;  // (the gate's strings have no error: unresolved is "")
    const size_t row = row_of((uint32_t)k);
    for (size_t o = 0; o < T; o++) {
      if (!((seen[row * W + o / 32] >> (o % 32)) & 1u)) continue;
      const char t = b.vout_tab[o].empty() ? 'C' : b.vout_tab[o][0];
      if (t == 'E') h.err[row * W + o / 32] |= 1u << (o % 32);
      else if (!(t == 'S' || t == 'F' || t == 'B' || t == 'N' || t == 'M')) h.oos[row * W + o / 32] |= 1u << (o % 32);
    }
  }
  h.truth.assign(ps.fconds.size() * W, 0);
  h.unk.assign(ps.fconds.size() * W, 0);
  for (size_t ci = 0; ci < ps.fconds.size(); ci++) {
    const CondRec& c = ps.fconds[ci];
    const size_t row = row_of(c.cstr);
    for (size_t o = 0; o < T; o++) {
      if (!((seen[row * W + o / 32] >> (o % 32)) & 1u)) continue;
      const std::string& oc = b.vout_tab[o];
      const char t = oc.empty() ? 'C' : oc[0];
      bool range = !(t == 'S' || t == 'F' || t == 'B' || t == 'N');  // a map / array, an error: outside the scope
      bool r = false;
      if (!range) {
        const PV v = outcome_value(oc);
        r = c.var_is_key ? cond_eval(c.op, v, c.other, &range) : cond_eval(c.op, c.other, v, &range);
      }
      if (range) h.unk[ci * W + o / 32] |= 1u << (o % 32);
      else if (r) h.truth[ci * W + o / 32] |= 1u << (o % 32);
    }
  }
  // the sets: row s of psets / dsets is foreach set s; entries carry the string's column
  auto col = [&](uint32_t c) { return ps.fkeys[ps.fconds[c].cstr].col; };
  for (const FeSet& s : ps.fsets) {
    h.sets.insert(h.sets.end(), {s.list, s.has_pre ? 1u : 0u, 0u, 0u});
    h.psets.push_back((uint32_t)(h.pents.size() / 2));
    h.psets.push_back((uint32_t)s.pre.any.size() | (s.pre.any_present ? 0x80000000u : 0u));
    h.psets.push_back((uint32_t)s.pre.all.size());
    h.psets.push_back(s.pre.const_false ? 1u : 0u);
    for (uint32_t c : s.pre.any) { h.pents.push_back(col(c)); h.pents.push_back(c); }
    for (uint32_t c : s.pre.all) { h.pents.push_back(col(c)); h.pents.push_back(c); }
    h.dsets.push_back((uint32_t)(h.dents.size() / 2));
    const size_t e0 = h.dents.size();
    for (uint32_t k : s.deny.strs) {
      const size_t e1 = h.dents.size();
      for (uint32_t c : s.deny.fold.any)
        if (ps.fconds[c].cstr == k) { h.dents.push_back(ps.fkeys[k].col); h.dents.push_back(c); }
      for (uint32_t c : s.deny.fold.all)
        if (ps.fconds[c].cstr == k) { h.dents.push_back(ps.fkeys[k].col); h.dents.push_back(c | KV_DENY_ALL); }
      if (h.dents.size() == e1) { h.dents.push_back(ps.fkeys[k].col); h.dents.push_back(KV_DENY_NOCOND); }
    }
    h.dsets.push_back((uint32_t)((h.dents.size() - e0) / 2));
    h.dsets.push_back(s.deny.fold.any_present ? 1u : 0u);
    h.dsets.push_back(s.deny.fold.const_false ? 1u : 0u);
  }
}

FeTables FeHost::view() const {
  FeTables t{};
  t.sets = sets.data(); t.lists = lists.data(); t.psets = psets.data(); t.pents = pents.data();
  t.dsets = dsets.data(); t.dents = dents.data(); t.outc = outc.data(); t.truth = truth.data();
  t.unk = unk.data(); t.err = err.data(); t.oos = oos.data(); t.el_res = el_res.data();
  t.el_ord = el_ord.data(); t.lstate = lstate.data();
  t.words = words;
  t.n_sets = (uint32_t)(sets.size() / 4);
  t.n_lists = (uint32_t)(lists.size() / 4);
  t.max_el = max_el;
  return t;
}

uint8_t foreach_fold_host(const FeHost& h, uint32_t set, uint64_t n_res, uint64_t r, uint32_t* elem) {
  const FeTables t = h.view();
  const uint32_t list = h.sets[4 * set];
  const uint32_t n_el = h.lists[4 * list + 1], el0 = h.lists[4 * list + 3];
  uint32_t key = FE_KEY_NONE;
  // the elements of store resource r: [first, ...) while el_res says r (what the kernel's
  // segments are made of)
  for (uint32_t e = h.first[(size_t)list * n_res + r]; e < n_el && h.el_res[el0 + e] == r; e++)
    key = std::min(key, kv_fe_key(kv_foreach_elem(t, set, e), h.el_ord[el0 + e]));
  if (elem) *elem = key < FE_KEY_PASS ? key >> 3 : 0xFFFFFFFFu;
  return (uint8_t)kv_fe_final(h.lstate[(size_t)list * n_res + r], key);
}

std::string foreach_error_host(const PolicySet& ps, const Batch& b, const FeHost& h, uint32_t set, uint64_t r,
                               uint32_t elem) {
  const FeSet& s = ps.fsets[set];
  const size_t K = ps.flist_keys[s.list].size();
  const size_t e = (size_t)h.first[(size_t)s.list * b.res.size() + r] + elem;
  for (uint32_t k : s.deny.order) {
    const std::string& o = b.vout_tab[b.fout[s.list][e * K + ps.fkeys[k].col]];
    if (!o.empty() && o[0] == 'E') return o.substr(1);
  }
  return std::string();
}

std::string deny_error_host(const PolicySet& ps, const Batch& b, uint32_t set, uint64_t r) {
  const size_t K = ps.vout_width(), k0 = ps.vkeys.size() + ps.ckeys.size();
  for (uint32_t k : ps.dsets[set].order) {
    const std::string& o = b.vout_tab[b.vout[r * K + k0 + k]];
    if (!o.empty() && o[0] == 'E') return o.substr(1);
  }
  return std::string();
}

}  // namespace kvh
