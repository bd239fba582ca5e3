// Rule preconditions: Go-exact condition evaluator, compile-time interning, per-batch truth
// tables (kvcond.h).
#include "kvcond.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "kvblocks.h"
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

// The interning tables a block compiles into (PolicySet::gate, deny or elem). strs (deny): every
// condition string of the block, those of conditions folded to a constant included.
struct CondSpace {
  CondIntern& in;
  std::vector<uint32_t>* strs;
  size_t any_strs = 0;  // how many of them the `any` list gave (it is compiled first)
  // foreach entries: `element` is a variable root too, and the strings are interned under
  // tag + text (the list and the resolver mode: PolicySet::elem.keys)
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
  auto ck = sp.in.key_id.find(text);
  if (ck == sp.in.key_id.end()) {
    ck = sp.in.key_id.emplace(text, (uint32_t)sp.in.keys.size()).first;
    sp.in.keys.push_back(text);
  }
  if (sp.strs) sp.strs->push_back(ck->second);
  if (op == CD_UNKNOWN) return 0;  // (deny: the string still has to resolve)
  CondRec c;
  c.op = op;
  c.var_is_key = kv;
  c.cstr = ck->second;
  c.other = kv ? value : key;
  const std::string id = std::to_string(op) + (kv ? "k" : "v") + std::to_string(c.cstr) + "|" + pv_key(c.other);
  auto it = sp.in.cond_id.find(id);
  if (it == sp.in.cond_id.end()) {
    it = sp.in.cond_id.emplace(id, (uint32_t)sp.in.conds.size()).first;
    sp.in.conds.push_back(std::move(c));
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
  const size_t ck0 = sp.in.keys.size(), cd0 = sp.in.conds.size();
  auto rollback = [&]() {
    sp.in.truncate(ck0, cd0);
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
    return sp.in.conds[a].cstr != sp.in.conds[b].cstr ? sp.in.conds[a].cstr < sp.in.conds[b].cstr : a < b;
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

// The `conditions` node of a deny map {conditions: <any / all block | old list>} (kyverno.Deny), -1
// for anything else: `deny: {}` and a missing or null `conditions` stay on the CPU route
int64_t deny_conditions(const JDoc& d, uint32_t node) {
  if (d.at(node).t != J_MAP) return -1;
  const JNode& n = d.at(node);
  int64_t cn = -1;
  for (uint32_t c = n.first; c < n.first + n.count; c++) {
    if (d.key(d.at(c)) != "conditions") return -1;
    cn = c;
  }
  return cn >= 0 && d.at((uint32_t)cn).t != J_NULL ? cn : -1;
}

// A deny block under the strict resolver into *out; *id: its interning key. False: outside the scope.
bool compile_deny_block(CondSpace sp, const JDoc& d, uint32_t node, DenySet* out, std::string* id) {
  DenySet& s = *out;
  sp.strs = &s.strs;
  bool always = false;
  if (!compile_block(sp, d, node, &s.fold, &always)) return false;
  // the strings in the order of the substitution's traversal with canonical key order, as for
  // pattern strings (kvvars.cpp): `all` before `any`, each list by index
  for (size_t i = sp.any_strs; i < s.strs.size(); i++) s.order.push_back(s.strs[i]);
  for (size_t i = 0; i < sp.any_strs; i++) s.order.push_back(s.strs[i]);
  std::sort(s.strs.begin(), s.strs.end());
  s.strs.erase(std::unique(s.strs.begin(), s.strs.end()), s.strs.end());
  *id = set_key(s.fold) + "#";
  for (uint32_t k : s.order) *id += std::to_string(k) + ",";
  return true;
}

}  // namespace

uint32_t compile_preconditions(PolicySet& ps, const JDoc& d, uint32_t node) {
  CondSpace sp{ps.gate, nullptr};
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
  const int64_t cn = deny_conditions(d, node);
  if (cn < 0) return 0;
  DenySet s;
  std::string id;
  if (!compile_deny_block(CondSpace{ps.deny, nullptr}, d, (uint32_t)cn, &s, &id)) return 0;
  auto it = ps.dset_id.find(id);
  if (it == ps.dset_id.end()) {
    it = ps.dset_id.emplace(id, (uint32_t)ps.dsets.size()).first;
    ps.dsets.push_back(std::move(s));
  }
  return it->second + 1;
}

namespace {
// interning text of a pattern document (key order as written)
void pattern_text(const PV& p, std::string* o) {
  switch (p.t) {
    case J_MAP:
      *o += '{';
      for (size_t i = 0; i < p.mk.size(); i++) {
        *o += std::to_string(p.mk[i].size()) + ":" + p.mk[i] + "=";
        pattern_text(p.mv[i], o);
      }
      *o += '}';
      break;
    case J_ARR:
      *o += '[';
      for (const PV& e : p.a) {
        pattern_text(e, o);
        *o += ',';
      }
      *o += ']';
      break;
    default: *o += pv_key(p); break;
  }
}
}  // namespace

namespace {
// a string below `node` that may hold an `element` variable (a superset: what makes an entry's
// strings depend on the entries before it)
bool may_read_element(const JDoc& d, uint32_t node) {
  const JNode& n = d.at(node);
  if (n.t == J_STR) {
    const std::string_view s = d.sval(n);
    return s.find("{{") != std::string_view::npos && s.find("element") != std::string_view::npos;
  }
  if (n.t == J_MAP || n.t == J_ARR)
    for (uint32_t c = n.first; c < n.first + n.count; c++)
      if (may_read_element(d, c)) return true;
  return false;
}

// a key or string below `node` that holds a `$(` reference
bool has_reference(const JDoc& d, uint32_t node) {
  const JNode& n = d.at(node);
  if (n.t == J_STR) return d.sval(n).find("$(") != std::string_view::npos;
  if (n.t == J_MAP || n.t == J_ARR)
    for (uint32_t c = n.first; c < n.first + n.count; c++) {
      if (n.t == J_MAP && d.key(d.at(c)).find("$(") != std::string_view::npos) return true;
      if (has_reference(d, c)) return true;
    }
  return false;
}

// One entry {list, preconditions?, deny | pattern} of validate.foreach, its element strings in
// the leak context `before` (the lists of the entries in front of it; empty for the first): 1 +
// its foreach set, 0 outside the scope (nothing is left behind)
uint32_t compile_foreach_entry(PolicySet& ps, const JDoc& d, uint32_t en, const FePatternCompiler* pattern,
                               const std::vector<uint32_t>& before, bool anypattern = false, bool patvars = false) {
  if (d.at(en).t != J_MAP) return 0;
  int64_t ln = -1, pn = -1, dn = -1, tn = -1, an = -1;
  for (uint32_t c = d.at(en).first; c < d.at(en).first + d.at(en).count; c++) {
    const std::string_view k = d.key(d.at(c));
    if (k == "list") ln = c;
    else if (k == "preconditions") pn = c;
    else if (k == "deny") dn = c;
    else if (k == "pattern" && pattern) tn = c;
    else if (k == "anyPattern" && pattern && anypattern) an = c;
    else return 0;  // context, ... (and pattern / anyPattern without their flags)
  }
  // an anyPattern entry (KV_COMPILE_FOREACH_ANYPATTERN): a list of 1 to 8 maps, nothing beside it
  // (an empty list passes with the rule message in the reference: left to it)
  if (an >= 0) {
    const JNode& al = d.at((uint32_t)an);
    if (tn >= 0 || dn >= 0 || al.t != J_ARR || al.count == 0 || al.count > FE_MAX_ALTS) return 0;
    for (uint32_t c = al.first; c < al.first + al.count; c++)
      if (d.at(c).t != J_MAP) return 0;
    // The reference substitutes the anyPattern list as one document (validation.go:560-567), so a
    // `$()` reference resolves against the list, alternative k at /k/...: an absolute one, or a
    // relative one that climbs above its alternative, does not resolve and every element is an
    // ERROR. The alternatives are compiled one by one here: a reference anywhere stays routed.
    if (has_reference(d, (uint32_t)an)) return 0;
  }
  // a pattern entry: the pattern a map, no deny beside it
  if (tn >= 0 && (dn >= 0 || d.at((uint32_t)tn).t != J_MAP)) return 0;
  if (ln < 0 || (dn < 0 && tn < 0 && an < 0) || d.at((uint32_t)ln).t != J_STR) return 0;
  const std::string list(d.sval(d.at((uint32_t)ln)));
  if (!list_query_in_scope(list)) return 0;
  if (pn >= 0 && d.at((uint32_t)pn).t == J_NULL) pn = -1;
  // the old list form of an entry's preconditions fails common.ToMap and is dropped by the
  // reference (validation.go:260-266): left to it
  if (pn >= 0 && d.at((uint32_t)pn).t != J_MAP) return 0;
  const int64_t cn = tn >= 0 || an >= 0 ? 0 : deny_conditions(d, (uint32_t)dn);
  if (cn < 0) return 0;
  // checkpoint: an entry outside the scope leaves nothing behind
  const size_t l0 = ps.flists.size(), k0 = ps.elem.keys.size(), c0 = ps.elem.conds.size();
  const size_t x0 = ps.fctx.size();
  auto drop_contexts = [&]() {  // (those this entry interned, the empty one included)
    for (; ps.fctx.size() > x0; ps.fctx.pop_back()) {
      std::string key;
      for (uint32_t l : ps.fctx.back()) key += std::to_string(l) + ",";
      ps.fctx_id.erase(key);
    }
  };
  auto rollback = [&]() {
    ps.elem.truncate(k0, c0);
    drop_contexts();
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
  // the leak context: that of the first entry unless a string of this one may read `element`
  // (KV_COMPILE_FOREACH_PATVARS: the strings of its pattern or alternatives are strings of the entry too)
  const bool pat_reads = patvars && ((tn >= 0 && may_read_element(d, (uint32_t)tn)) || (an >= 0 && may_read_element(d, (uint32_t)an)));
  if (!before.empty() &&
      ((pn >= 0 && may_read_element(d, (uint32_t)pn)) || (dn >= 0 && may_read_element(d, (uint32_t)dn)) || pat_reads)) {
    if (ps.fctx.empty()) {
      ps.fctx.emplace_back();
      ps.fctx_id.emplace(std::string(), 0u);
    }
    std::string key;
    for (uint32_t l : before) key += std::to_string(l) + ",";
    auto ci = ps.fctx_id.find(key);
    if (ci == ps.fctx_id.end()) {
      ci = ps.fctx_id.emplace(key, (uint32_t)ps.fctx.size()).first;
      ps.fctx.push_back(before);
    }
    s.ctx = ci->second;
  }
  const std::string at = s.ctx ? "@" + std::to_string(s.ctx) : std::string();
  CondSpace sp{ps.elem, nullptr};
  sp.element = true;
  if (pn >= 0) {
    bool always = false;
    sp.tag = "p" + std::to_string(s.list) + at + ":";
    if (!compile_block(sp, d, (uint32_t)pn, &s.pre, &always)) return rollback();
    s.has_pre = !always;
    if (always) s.pre = CondSet();
  }
  sp.tag = "d" + std::to_string(s.list) + at + ":";
  std::string did;
  if (tn >= 0) {
    did = "P";
    pattern_text(to_pv(d, (uint32_t)tn), &did);
  } else if (an >= 0) {  // (an any set is interned by its alternatives' texts, in order)
    did = "A";
    pattern_text(to_pv(d, (uint32_t)an), &did);
  } else if (!compile_deny_block(sp, d, (uint32_t)cn, &s.deny, &did)) {
    return rollback();
  }
  // (a set that kept no string of its context reads nothing the entries before it left: the first entry's set)
  if (s.ctx && !s.has_pre && s.deny.strs.empty() && !pat_reads) {
    s.ctx = 0;
    if (ps.elem.keys.size() == k0) drop_contexts();  // (no string names the context either)
  }
  const std::string id = std::to_string(s.list) + (s.ctx ? "@" + std::to_string(s.ctx) : std::string()) + "|" +
                         (s.has_pre ? set_key(s.pre) : std::string("none")) + "|" + did;
  auto it = ps.fset_id.find(id);
  // a pattern entry met for the first time: its program, rooted at the list's element
  if (tn >= 0 && it == ps.fset_id.end()) {
    if (!(*pattern)((uint32_t)tn, list, s.list, &s)) return rollback();
    s.pattern = true;
    s.pat = (uint32_t)ps.fpats.size();
    ps.fpats.push_back((uint32_t)ps.fsets.size());
  }
  // an anyPattern entry met for the first time: one plain pattern program per alternative, each
  // with a root pattern node of its own (the caller's checkpoint takes back what the earlier
  // alternatives of a refused entry left)
  if (an >= 0 && it == ps.fset_id.end()) {
    const JNode& al = d.at((uint32_t)an);
    for (uint32_t c = al.first; c < al.first + al.count; c++) {
      FeSet alt;
      alt.list = s.list;
      alt.ctx = s.ctx;
      if (!(*pattern)(c, list, s.list, &alt)) return rollback();
      s.alt_prog.push_back(alt.prog);
      s.alt_root.push_back(alt.root_pnode);
      s.vorder.insert(s.vorder.end(), alt.vorder.begin(), alt.vorder.end());
    }
    s.any = true;
    s.anyi = (uint32_t)ps.fanys.size();
    ps.fanys.push_back((uint32_t)ps.fsets.size());
  }
  // the strings this entry added: their list, resolver mode and column in the list's element rows
  for (size_t i = ps.fkeys.size(); i < ps.elem.keys.size(); i++) {
    const std::string& t = ps.elem.keys[i];
    FeKey k;
    k.list = s.list;
    k.precond = t[0] == 'p';
    const size_t colon = t.find(':'), ctx_at = t.find('@');
    if (ctx_at < colon) k.ctx = (uint32_t)std::stoul(t.substr(ctx_at + 1, colon - ctx_at - 1));
    k.text = t.substr(colon + 1);
    k.col = (uint32_t)ps.flist_keys[s.list].size();
    ps.flist_keys[s.list].push_back((uint32_t)i);
    ps.fkeys.push_back(std::move(k));
  }
  if (it == ps.fset_id.end()) {
    it = ps.fset_id.emplace(id, (uint32_t)ps.fsets.size()).first;
    ps.fsets.push_back(std::move(s));
  }
  return it->second + 1;
}

// the sizes every table a foreach rule compiles into had before it, and the way back
struct FeCheckpoint {
  PolicySet& ps;
  size_t prog, fix, pnodes, lists, keys, conds, fkeys, sets, pats, anys, ctxs, paths;
  size_t preds, alts, conjs, atoms, gsegs, gwords, strs;  // (what the programs' leaf predicates interned)
  std::vector<size_t> list_keys;
  std::vector<bool> path_set;
  explicit FeCheckpoint(PolicySet& p)
      : ps(p), prog(p.prog.size()), fix(p.slot_fix.size()), pnodes(p.pnodes.size()), lists(p.flists.size()),
        keys(p.elem.keys.size()), conds(p.elem.conds.size()), fkeys(p.fkeys.size()), sets(p.fsets.size()),
        pats(p.fpats.size()), anys(p.fanys.size()), ctxs(p.fctx.size()), paths(p.fchains.size()), preds(p.preds.size()), alts(p.alts.size()),
        conjs(p.conjs.size()), atoms(p.atoms.size()), gsegs(p.gsegs.size()), gwords(p.gwords.size()), strs(p.strs.size()) {
    for (const auto& k : p.flist_keys) list_keys.push_back(k.size());
    for (const FeChain& c : p.fchains) path_set.push_back(!c.steps.empty());
  }
  template <class M>
  static void drop_from(M& ids, size_t n0) {
    for (auto it = ids.begin(); it != ids.end();) it = it->second >= n0 ? ids.erase(it) : std::next(it);
  }
  void rollback() {
    ps.prog.resize(prog);
    ps.slot_fix.resize(fix);
    ps.pnodes.resize(pnodes);
    ps.preds.resize(preds);
    drop_from(ps.pred_cache, preds);
    ps.alts.resize(alts);
    ps.conjs.resize(conjs);
    ps.atoms.resize(atoms);
    ps.gsegs.resize(gsegs);
    ps.gwords.resize(gwords);
    ps.strs.resize(strs);
    ps.elem.truncate(keys, conds);
    ps.fkeys.resize(fkeys);
    ps.flists.resize(lists);
    ps.flist_keys.resize(lists);
    for (size_t l = 0; l < lists; l++) ps.flist_keys[l].resize(list_keys[l]);
    drop_from(ps.flist_id, lists);
    ps.fsets.resize(sets);
    drop_from(ps.fset_id, sets);
    ps.fpats.resize(pats);
    ps.fanys.resize(anys);
    ps.fctx.resize(ctxs);
    drop_from(ps.fctx_id, ctxs);
    ps.fchains.resize(paths);
    for (size_t l = 0; l < paths; l++)
      if (!path_set[l]) ps.fchains[l] = FeChain();
  }
};
}  // namespace

uint32_t compile_foreach(PolicySet& ps, const JDoc& d, uint32_t node, const FePatternCompiler* pattern, uint32_t* chain,
                         bool anypattern, bool patvars) {
  // validate.foreach: a list of one entry, or (chain: KV_COMPILE_FOREACH_ENTRIES) of 2 to 16, each
  // what a single entry may be. With several, keys of entry k-1's last element leak into entry
  // k's `element` (kvcond.h): entry k's strings are compiled in the context of the lists before it
  if (chain) *chain = 0;
  if (d.at(node).t != J_ARR) return 0;
  const uint32_t count = d.at(node).count, first = d.at(node).first;
  if (count == 1 && !(anypattern && d.at(first).t == J_MAP && d.get(first, "anyPattern") >= 0))
    return compile_foreach_entry(ps, d, first, pattern, {}, false, patvars);
  if (count == 1) {  // (an anyPattern entry refused at a later alternative: the earlier ones' programs go)
    FeCheckpoint ck(ps);
    const uint32_t s = compile_foreach_entry(ps, d, first, pattern, {}, true, patvars);
    if (!s) ck.rollback();
    return s;
  }
  if (!chain || count < 2 || count > FE_MAX_ENTRIES) return 0;
  FeCheckpoint ck(ps);
  std::vector<uint32_t> sets, before;
  std::string id;
  for (uint32_t en = first; en < first + count; en++) {
    const uint32_t s = compile_foreach_entry(ps, d, en, pattern, before, anypattern, patvars);
    if (!s) {
      ck.rollback();
      return 0;
    }
    sets.push_back(s - 1);
    before.push_back(ps.fsets[s - 1].list);
    id += std::to_string(s - 1) + ",";
  }
  auto it = ps.fe_chain_id.find(id);
  if (it == ps.fe_chain_id.end()) {
    it = ps.fe_chain_id.emplace(id, (uint32_t)ps.fe_chains.size()).first;
    ps.fe_chains.push_back(std::move(sets));
  }
  *chain = it->second + 1;
  return 0;
}

// ------------------------------------------------------------------ per batch
namespace {

// One string row of a space's planes: its outcome ids are outc[at .. at + n); strict: resolved
// under the strict resolver (its error and out-of-scope planes are filled)
struct StrRow {
  size_t at, n;
  bool strict;
};

// One block to pack: its fold and (deny) every string of it, sorted; without strs the strings
// are those of the fold's conditions
struct BlockRef {
  const CondSet* fold;
  const std::vector<uint32_t>* strs;
};

// dst[c * n + i] = src[i * stride + col0 + c]: outcome rows to [string][item] (a lane's load is coalesced)
void transpose(const uint32_t* src, size_t stride, size_t col0, size_t cols, size_t n, uint32_t* dst) {
  for (size_t i = 0; i < n; i++)
    for (size_t c = 0; c < cols; c++) dst[c * n + i] = src[i * stride + col0 + c];
}

// The sets and entries of `blocks` into h: per block one run of entries per string, in string
// order: the string's `any` conditions, its `all` conditions, or a bare entry where no condition of
// the string is left to evaluate. key_col: the string row an entry names, per string of the space.
void pack_sets(const std::vector<CondRec>& conds, const std::vector<BlockRef>& blocks, const std::vector<uint32_t>& key_col,
               CondHost* h) {
  std::vector<uint32_t> own;
  for (const BlockRef& b : blocks) {
    const CondSet& s = *b.fold;
    if (!b.strs) {
      own.clear();
      for (uint32_t c : s.any) own.push_back(conds[c].cstr);
      for (uint32_t c : s.all) own.push_back(conds[c].cstr);
      std::sort(own.begin(), own.end());
      own.erase(std::unique(own.begin(), own.end()), own.end());
    }
    const size_t e0 = h->ents.size();
    for (uint32_t k : b.strs ? *b.strs : own) {
      const size_t e1 = h->ents.size();
      for (uint32_t c : s.any)
        if (conds[c].cstr == k) h->ents.insert(h->ents.end(), {key_col[k], c});
      for (uint32_t c : s.all)
        if (conds[c].cstr == k) h->ents.insert(h->ents.end(), {key_col[k], c | KV_ENT_ALL});
      if (h->ents.size() == e1) h->ents.insert(h->ents.end(), {key_col[k], KV_ENT_NOCOND});
    }
    h->sets.insert(h->sets.end(), {(uint32_t)(e0 / 2), (uint32_t)((h->ents.size() - e0) / 2),
                                   (s.any_present ? KV_SET_ANY : 0u) | (s.const_false ? KV_SET_FALSE : 0u), 0u});
  }
}

// The planes of h over the outcome ids already in h->outc: per condition the truth / unknown
// planes over the outcomes its string (row key_row[cstr]) takes in this batch, and per strict
// string row the outcomes that are a substitution error / outside the device scope (no such
// planes when no row is strict).
void fill_planes(const Batch& b, const std::vector<CondRec>& conds, const std::vector<uint32_t>& key_row,
                 const std::vector<StrRow>& rows, CondHost* h) {
  const size_t T = b.vout_tab.size();
  const uint32_t W = (uint32_t)std::max<size_t>((T + 31) / 32, 1);
  h->words = W;
  auto set = [&](std::vector<uint32_t>& plane, size_t row, size_t o) { plane[row * W + o / 32] |= 1u << (o % 32); };
  // the outcomes each string takes in this batch
  std::vector<uint32_t> seen(rows.size() * W, 0);
  bool strict = false;
  for (size_t r = 0; r < rows.size(); r++) {
    for (size_t i = 0; i < rows[r].n; i++) set(seen, r, h->outc[rows[r].at + i]);
    strict |= rows[r].strict;
  }
  auto taken = [&](size_t row, size_t o) { return ((seen[row * W + o / 32] >> (o % 32)) & 1u) != 0u; };
  auto tag = [&](size_t o) { return b.vout_tab[o].empty() ? 'C' : b.vout_tab[o][0]; };
  if (strict) {
    h->err.assign(rows.size() * W, 0);
    h->oos.assign(rows.size() * W, 0);
    for (size_t r = 0; r < rows.size(); r++)
      for (size_t o = 0; o < T && rows[r].strict; o++) {
        if (!taken(r, o)) continue;
        const char t = tag(o);
        if (t == 'E') set(h->err, r, o);
        else if (!(t == 'S' || t == 'F' || t == 'B' || t == 'N' || t == 'M')) set(h->oos, r, o);
      }
  }
  h->truth.assign(conds.size() * W, 0);
  h->unk.assign(conds.size() * W, 0);
  for (size_t ci = 0; ci < conds.size(); ci++) {
    const CondRec& c = conds[ci];
    for (size_t o = 0; o < T; o++) {
      if (!taken(key_row[c.cstr], o)) continue;
      const char t = tag(o);
      bool range = !(t == 'S' || t == 'F' || t == 'B' || t == 'N');  // a map / array, an error: outside the scope
      bool r = false;
      if (!range) {
        const PV v = outcome_value(b.vout_tab[o]);
        r = c.var_is_key ? cond_eval(c.op, v, c.other, &range) : cond_eval(c.op, c.other, v, &range);
      }
      if (range) set(h->unk, ci, o);
      else if (r) set(h->truth, ci, o);
    }
  }
}

// The blocks of a space whose strings resolve per resource into columns [k0, k0 + keys) of the
// outcome rows (the preconditions, the deny blocks): string row = string.
void build_blocks(const PolicySet& ps, const Batch& b, const CondIntern& in, size_t k0, bool strict,
                  const std::vector<BlockRef>& blocks, CondHost* h) {
  *h = CondHost();
  if (blocks.empty()) return;
  const size_t n = b.res.size(), K = ps.vout_width(), C = in.keys.size();
  if (b.vout.size() != K * n) throw std::runtime_error("condition blocks: outcome rows do not match the policy set");
  h->outc.resize(C * n);
  transpose(b.vout.data(), K, k0, C, n, h->outc.data());
  std::vector<uint32_t> ident(C);
  std::vector<StrRow> rows(C);
  for (size_t c = 0; c < C; c++) {
    ident[c] = (uint32_t)c;
    rows[c] = {c * n, n, strict};
  }
  pack_sets(in.conds, blocks, ident, h);
  fill_planes(b, in.conds, ident, rows, h);
}

// the error of the first string of `order` whose outcome (outcome_of(string)) is a substitution error
template <class F>
std::string first_error(const Batch& b, const std::vector<uint32_t>& order, F outcome_of) {
  for (uint32_t k : order) {
    const std::string& o = b.vout_tab[outcome_of(k)];
    if (!o.empty() && o[0] == 'E') return o.substr(1);
  }
  return std::string();
}

}  // namespace

CondBlocks CondHost::view() const {
  return CondBlocks{sets.data(), ents.data(), outc.data(), truth.data(), unk.data(), err.data(), oos.data(), words};
}

void build_pre(const PolicySet& ps, const Batch& b, CondHost* out) {
  std::vector<BlockRef> blocks;
  for (const CondSet& s : ps.csets) blocks.push_back({&s, nullptr});
  build_blocks(ps, b, ps.gate, ps.vkeys.size(), false, blocks, out);
}

void build_deny(const PolicySet& ps, const Batch& b, CondHost* out) {
  std::vector<BlockRef> blocks;
  for (const DenySet& s : ps.dsets) blocks.push_back({&s.fold, &s.strs});
  build_blocks(ps, b, ps.deny, ps.vkeys.size() + ps.gate.keys.size(), true, blocks, out);
}

uint8_t pre_status_host(const CondHost& h, uint32_t set, uint64_t n_res, uint64_t r) {
  return (uint8_t)kv_gate_status(kv_cond_fold<false>(h.view(), set, n_res, r));
}

uint8_t deny_status_host(const CondHost& h, uint32_t set, uint64_t n_res, uint64_t r) {
  return (uint8_t)kv_deny_status(kv_cond_fold<true>(h.view(), set, n_res, r));
}

std::string deny_error_host(const PolicySet& ps, const Batch& b, uint32_t set, uint64_t r) {
  const size_t K = ps.vout_width(), k0 = ps.vkeys.size() + ps.gate.keys.size();
  return first_error(b, ps.dsets[set].order, [&](uint32_t k) { return b.vout[r * K + k0 + k]; });
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
  // per list: the element blocks, [string][element] outcome ids, the per-resource state; a string
  // row per (list, string of the list)
  h.lstate.resize(L * n);
  h.first.resize(L * n);
  std::vector<StrRow> rows;
  std::vector<uint32_t> key_col(ps.fkeys.size()), key_row(ps.fkeys.size());
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
    const uint32_t o0 = (uint32_t)h.deny.outc.size();
    h.deny.outc.resize(o0 + (size_t)n_el * K);
    transpose(b.fout[l].data(), K, 0, K, n_el, h.deny.outc.data() + o0);
    h.lists.insert(h.lists.end(), {o0, n_el, (uint32_t)rows.size(), el0});
    for (size_t c = 0; c < K; c++) {
      const uint32_t k = ps.flist_keys[l][c];
      key_col[k] = (uint32_t)c;
      key_row[k] = (uint32_t)rows.size();
      // (the gate's strings have no error: unresolved is "")
      rows.push_back({o0 + c * n_el, n_el, !ps.fkeys[k].precond});
    }
    h.max_el = std::max(h.max_el, n_el);
  }
  fill_planes(b, ps.elem.conds, key_row, rows, &h.deny);
  h.deny.err.resize(rows.size() * h.deny.words);  // (a row per string even where none is strict:
  h.deny.oos.resize(rows.size() * h.deny.words);  // kv_foreach_elem offsets the planes by list)
  // the sets: row s of gate / deny is foreach set s; entries carry the string's column
  std::vector<BlockRef> gate, deny;
  for (const FeSet& s : ps.fsets) {
    // (a pattern set: an empty deny row, never folded; word 2 names its pattern set)
    // (an any set likewise; word 3 names it)
    h.sets.insert(h.sets.end(), {s.list, s.has_pre ? 1u : 0u, s.pattern ? 1u + s.pat : 0u, s.any ? 1u + s.anyi : 0u});
    gate.push_back({&s.pre, nullptr});
    deny.push_back({&s.deny.fold, &s.deny.strs});
  }
  pack_sets(ps.elem.conds, gate, key_col, &h.gate);
  pack_sets(ps.elem.conds, deny, key_col, &h.deny);
  // the rules of several entries: per chain its entries' sets
  for (const std::vector<uint32_t>& c : ps.fe_chains) {
    h.chains.insert(h.chains.end(), {(uint32_t)h.chain_ents.size(), (uint32_t)c.size()});
    h.chain_ents.insert(h.chain_ents.end(), c.begin(), c.end());
  }
  // the pattern sets: their program and the path to their list's elements
  for (uint32_t fs : ps.fpats) {
    const FeSet& s = ps.fsets[fs];
    const FeChain& c = ps.fchains.at(s.list);
    h.pats.insert(h.pats.end(), {fs, s.prog, (uint32_t)(h.chain.size() / 2), (uint32_t)(c.words.size() / 2)});
    h.chain.insert(h.chain.end(), c.words.begin(), c.words.end());
  }
  // the any sets: their alternatives' programs and the path to their list's elements
  for (uint32_t fs : ps.fanys) {
    const FeSet& s = ps.fsets[fs];
    const FeChain& c = ps.fchains.at(s.list);
    h.anys.insert(h.anys.end(), {fs, (uint32_t)h.any_alts.size(), (uint32_t)s.alt_prog.size(), (uint32_t)(h.chain.size() / 2),
                                 (uint32_t)(c.words.size() / 2), 0u, 0u, 0u});
    h.any_alts.insert(h.any_alts.end(), s.alt_prog.begin(), s.alt_prog.end());
    h.chain.insert(h.chain.end(), c.words.begin(), c.words.end());
  }
  // pattern variables in entries (KV_COMPILE_FOREACH_PATVARS): per pattern set, then per any set,
  // the run of its strings' rows in substitution order, and the plane of the outcomes that are a
  // map or an array (beside err / oos, which fill_planes gave the strict rows)
  if (ps.n_vpats || ps.n_vanys) {
    for (const std::vector<uint32_t>* v : {&ps.fpats, &ps.fanys})
      for (uint32_t fs : *v) {
        const FeSet& s = ps.fsets[fs];
        h.vruns.insert(h.vruns.end(), {(uint32_t)h.vrows.size(), (uint32_t)s.vorder.size()});
        for (uint32_t k : s.vorder) h.vrows.push_back(ps.fkeys[k].col);
      }
    const uint32_t W = h.deny.words;
    h.mpl.assign(rows.size() * W, 0);
    for (size_t r = 0; r < rows.size(); r++)
      for (size_t i = 0; i < rows[r].n && rows[r].strict; i++) {
        const uint32_t o = h.deny.outc[rows[r].at + i];
        if (!b.vout_tab[o].empty() && b.vout_tab[o][0] == 'M') h.mpl[r * W + o / 32] |= 1u << (o % 32);
      }
  }
}

FeVarTables FeHost::var_view(const uint32_t* ityp) const {
  return FeVarTables{vruns.data(), vrows.data(), mpl.data(), ityp};
}

uint32_t foreach_subst_host(const FeHost& h, uint32_t set, uint64_t n_res, uint64_t r, uint32_t elem) {
  const uint32_t pat = h.sets[4 * set + 2], any = h.sets[4 * set + 3];
  if (!h.has_vars() || (!pat && !any)) return 0;
  const size_t run = pat ? pat - 1 : h.pats.size() / 4 + (any - 1);
  const FeTables t = h.view();
  const FeVarTables v = h.var_view(nullptr);
  const uint32_t list = h.sets[4 * set];
  return kv_fe_subst(t, v, h.lists.data() + 4 * list, h.vruns[2 * run], h.vruns[2 * run + 1],
                     h.first[(size_t)list * n_res + r] + elem);
}

uint32_t foreach_elem_outcome(const PolicySet& ps, const Batch& b, const FeHost& h, uint32_t key, uint64_t r, uint32_t elem) {
  const FeKey& k = ps.fkeys[key];
  const size_t K = ps.flist_keys[k.list].size();
  const size_t e = (size_t)h.first[(size_t)k.list * b.res.size() + r] + elem;
  return b.fout[k.list][e * K + k.col];
}

std::string foreach_subst_error_host(const PolicySet& ps, const Batch& b, const FeHost& h, uint32_t set, uint64_t r,
                                     uint32_t elem) {
  return first_error(b, ps.fsets[set].vorder, [&](uint32_t k) { return foreach_elem_outcome(ps, b, h, k, r, elem); });
}

FeTables FeHost::view() const {
  FeTables t{};
  t.sets = sets.data(); t.lists = lists.data(); t.el_res = el_res.data(); t.el_ord = el_ord.data();
  t.lstate = lstate.data();
  t.deny = deny.view();
  t.gate = t.deny;
  t.gate.sets = gate.sets.data();
  t.gate.ents = gate.ents.data();
  t.n_sets = (uint32_t)(sets.size() / 4);
  t.n_lists = (uint32_t)(lists.size() / 4);
  t.max_el = max_el;
  t.chains = chains.data(); t.chain_ents = chain_ents.data();
  t.n_chains = (uint32_t)(chains.size() / 2);
  return t;
}

FePatTables FeHost::pat_view() const {
  return FePatTables{pats.data(), chain.data(), first.data(), (uint32_t)(pats.size() / 4)};
}

FeAnyTables FeHost::any_view() const {
  return FeAnyTables{anys.data(), any_alts.data(), chain.data(), first.data(), (uint32_t)(anys.size() / 8),
                     (uint32_t)any_alts.size()};
}

uint8_t foreach_fold_host(const FeHost& h, uint32_t set, uint64_t n_res, uint64_t r, uint32_t* elem) {
  // (a pattern set's elements are walked on the device only: no host evaluator)
  if (h.sets[4 * set + 2] || h.sets[4 * set + 3])
    throw std::runtime_error("foreach_fold_host: a pattern set or any set has no host fold");
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

uint8_t foreach_chain_fold_host(const FeHost& h, uint32_t chain, uint64_t n_res, uint64_t r, uint32_t* entry, uint32_t* elem,
                                FeChainScratch* scratch) {
  // the entry sets' rows of this resource (what kv_foreach_fin_kernel's input holds) up to the
  // entry that ends the walk, then the lane body of kv_foreach_chain_kernel over them
  FeChainScratch own;
  FeChainScratch& sc = scratch ? *scratch : own;
  const uint32_t e0 = h.chains[2 * chain], n_ent = h.chains[2 * chain + 1];
  if (sc.acc.empty()) {  // (one resource: the rows have a stride of 1)
    sc.acc.assign(h.sets.size() / 4, FE_KEY_NONE);
    sc.ls.resize(h.lists.size() / 4);
  }
  for (size_t l = 0; l < sc.ls.size(); l++) sc.ls[l] = h.lstate[l * n_res + r];
  for (uint32_t k = 0; k < n_ent; k++) {
    const uint32_t s = h.chain_ents[e0 + k];
    if (sc.ls[h.sets[4 * s]] == FE_LIST_OOS) break;  // (the walk stops here: nothing behind is read)
    uint32_t e = 0xFFFFFFFFu;
    const uint8_t st = foreach_fold_host(h, s, n_res, r, &e);
    sc.acc[s] = st == ST_PASS ? FE_KEY_PASS : st == ST_SKIP ? FE_KEY_NONE : (e << 3 | st);
    if (sc.acc[s] < FE_KEY_PASS) break;
  }
  FeTables t = h.view();  // (pointers only)
  t.lstate = sc.ls.data();
  uint32_t key = FE_KEY_NONE;
  const uint8_t st = (uint8_t)kv_fe_chain(t, chain, 1, 0, sc.acc.data(), &key);
  for (uint32_t k = 0; k < n_ent; k++) sc.acc[h.chain_ents[e0 + k]] = FE_KEY_NONE;
  if (entry) *entry = key < FE_KEY_PASS ? key >> 19 : 0xFFFFFFFFu;
  if (elem) *elem = key < FE_KEY_PASS && (key & 7u) != ST_CPU ? (key >> 3) & 0xFFFFu : 0xFFFFFFFFu;
  return st;
}

std::string foreach_error_host(const PolicySet& ps, const Batch& b, const FeHost& h, uint32_t set, uint64_t r,
                               uint32_t elem) {
  const FeSet& s = ps.fsets[set];
  const size_t K = ps.flist_keys[s.list].size();
  const size_t e = (size_t)h.first[(size_t)s.list * b.res.size() + r] + elem;
  return first_error(b, s.deny.order, [&](uint32_t k) { return b.fout[s.list][e * K + ps.fkeys[k].col]; });
}

}  // namespace kvh
