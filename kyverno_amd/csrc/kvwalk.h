// The pattern walk: the uniform-pc SIMT interpreter over the structured program of kvcompile.cpp
// (validate.go:29-194, anchor.go:21-277), one copy for its two callers:
//   kv_validate_kernel (ELEM = false): a lane is a resource, the root its root node;
//   kv_foreach_pat_kernel (ELEM = true, KV_COMPILE_FOREACH_PATTERN): a lane is an element of a
//   foreach list, the root that element's node (MatchPattern(element, pattern): the element map
//   as the whole resource), kv_foreach_any_kernel (KV_COMPILE_FOREACH_ANYPATTERN: the same, once per
//   alternative of an anyPattern entry), kv_foreach_patv_kernel / kv_foreach_anyv_kernel (ELEM and
//   VARS, KV_COMPILE_FOREACH_PATVARS: the two with `{{element...}}` strings in the patterns: a
//   dynamic leaf reads the element's substituted value), and the host harness tools/kvemu (a
//   one-lane wave).
// Lanes that skip a subtree (absent anchored key) or raise an error park on a wake-up pc (the scope
// end / catch point) instead of branching, so the wave never diverges in program position; loops
// over resource arrays run max(len) uniform iterations with the counter in LDS per wave.
//
// A node's index is row * KV_LANES + the lane of its *resource* in the wave-group layout
// (kv_layout.h). With a lane per resource that is the lane itself (kvdevfn.h ni()); with a lane
// per element it is `rl`, the resource's index modulo KV_LANES, passed in.
//
// ELEM only: the element comes out of the JSON context, so the reference compares every number of
// it as float64, where the store types a literal int64 (Val::type == NT_INT). The compiler marks
// the leaves whose verdict depends on that typing (OP_LEAF aux 1: a string pattern compared on
// the number's text form); a lane that meets an NT_INT value at such a leaf, or an NT_INT value
// of magnitude >= 2^53 at any leaf, sets `cpu`: its element is ST_CPU whatever the walk says.
// Needs kvdevfn.h; the caller owns the LDS arrays (s_cur[KV_MAXD][KV_WG], s_lfirst / s_llen
// [KV_MAXL][KV_WG], s_li[KV_WG / 64][KV_MAXL]).
#pragma once

#define KV_MAXD 16  // cursor levels (pattern depth + 1)
#define KV_MAXL 4   // nested array levels

template <bool ELEM>
__device__ __forceinline__ uint32_t kv_nix(uint32_t row, uint32_t rl) {
  return ELEM ? row * KV_LANES + rl : ni(row);
}

// lookup_op (kvdevfn.h) for a lane whose resource sits in lane rl of its rows
template <bool ELEM>
__device__ __forceinline__ uint32_t kv_lookup_op(const Node* __restrict__ N, uint32_t m, uint32_t a, uint32_t aux, uint32_t rl) {
  if (!ELEM) return lookup_op(N, m, a, aux);
  if (m == ABSENT) return ABSENT;
  const Node n = N[m];
  if (node_type(n.kt) != NT_MAP) return ABSENT;
  if (aux & AUX_SCAN) {  // keep-all map: scan for the key id
    for (uint32_t i = 0; i < n.b; i++)
      if (node_key(N[kv_nix<ELEM>(n.a + i, rl)].kt) == a) return kv_nix<ELEM>(n.a + i, rl);
    return ABSENT;
  }
  if (a >= n.b) return ABSENT;
  const uint32_t c = kv_nix<ELEM>(n.a + a, rl);
  return node_type(N[c].kt) == NT_ABSENT ? ABSENT : c;
}

// an int64-typed value whose float64 reading the device cannot stand in for at this leaf
__device__ __forceinline__ bool kv_int_unsafe(const DevBatch& B, const Node& n, bool sensitive) {
  if (node_type(n.kt) != NT_INT) return false;
  if (sensitive) return true;
  const int64_t i = B.vals[n.a].i;
  return i >= (1ll << 53) || i <= -(1ll << 53);
}

// Runs the program at *prog (a wave-uniform word) for the lanes with `run` set, from node `root`.
// r: the lane's resource (the dynamic leaves' row); rl: see above (ELEM only). st and e: the
// lane's status and error fields, written by the lanes that ran (MatchPattern's epilogue,
// validate.go:29-50). cpu (ELEM only): see above.
// VARS (ELEM only; KV_COMPILE_FOREACH_PATVARS, kvforeach.h FeVarTables): a dynamic leaf's row is the
// lane's *element*: the predicate id is vrow[a * vstride + ve], the outcome of string row a of the
// element's list on element ve, evaluated on the batch predicate table as the resource arm does;
// the int-typing guard is decided per substituted value, by the outcome's bit in `ityp`.
template <bool ELEM, bool VARS = false>
__device__ __forceinline__ void kv_walk(const DevPS& P, const DevBatch& B, const Node* __restrict__ N,
                                        const uint32_t* __restrict__ prog, uint32_t root, bool run, uint32_t r,
                                        uint32_t n_res, uint32_t rl, uint32_t (*s_cur)[KV_WG],
                                        uint32_t (*s_lfirst)[KV_WG], uint32_t (*s_llen)[KV_WG],
                                        uint32_t (*s_li)[KV_MAXL], uint32_t& st, EState& e, bool& cpu,
                                        const uint32_t* __restrict__ vrow = nullptr, uint32_t vstride = 0u,
                                        uint32_t ve = 0u, const uint32_t* __restrict__ ityp = nullptr) {
  const uint32_t lane = threadIdx.x;
  const uint32_t wv = lane >> 6;
  if (__ballot(run)) {
    uint64_t areg = 0, apres = 0;
    uint32_t keynode = ABSENT;
    uint32_t wait = run ? 0u : KV_SENT;
    uint32_t pc = uni(*prog);
    s_cur[0][lane] = root;
    auto raise = [&](uint32_t kind, uint32_t pn, uint32_t rn, uint32_t cpc) {
      e.kind = kind;
      e.flags = 0;
      e.pn = pn;
      e.res = rn;
      e.key = keynode;
      e.i0 = s_li[wv][0];
      e.i1 = s_li[wv][1];
      e.i2 = s_li[wv][2];
      e.i3 = s_li[wv][3];
      wait = cpc;
    };
    uint32_t guard = 0;
    while (true) {
      // every program terminates (forward pcs, loops bounded by array lengths);
      // the guard only turns an interpreter bug into a CPU-routed verdict instead of a hung wave
      if (++guard > (1u << 24)) {
        if (wait != KV_SENT) st = ST_CPU;
        break;
      }
      if (wait == pc) wait = 0;
      if (!__ballot(wait == 0)) {
        const uint32_t m = uni(wave_min(wait));
        if (m == KV_SENT) break;
        pc = m;
        continue;
      }
      const Inst& in = P.prog[pc];
      const uint32_t opw = uni(in.op);
      const uint32_t op = opw & 0xFF;
      const uint32_t d = (opw >> 8) & 0xFF;
      const uint32_t aux = (opw >> 16) & 0xFF;
      const uint32_t ia = uni(in.a), ib = uni(in.b), ic = uni(in.c);
      const bool A = wait == 0;
      uint32_t next = pc + 1;
      switch (op) {
        case OP_MAPCHK:
        case OP_ARRCHK:
          if (A) {
            const uint32_t v = s_cur[d][lane];
            const uint32_t want = op == OP_MAPCHK ? NT_MAP : NT_ARR;
            if (v == ABSENT || node_type(N[v].kt) != want) raise(op == OP_MAPCHK ? E_TYPE_MAP : E_TYPE_ARR, ia, v, ic);
          }
          break;
        case OP_AREG:
          if (A) {
            areg |= 1ull << (aux & 63);
            if (kv_lookup_op<ELEM>(N, s_cur[d][lane], ia, aux, rl) != ABSENT) apres |= 1ull << (aux & 63);
          }
          break;
        case OP_KEY:
        case OP_KEYV:
          if (A) {
            const uint32_t c = kv_lookup_op<ELEM>(N, s_cur[d][lane], ia, aux, rl);
            s_cur[d + 1][lane] = c;
            if (op == OP_KEY && c == ABSENT) wait = ib;
          }
          break;
        case OP_KEYGLOB:
          if (A) {
            if constexpr (ELEM) {  // (no metadata site in an entry's pattern: the compiler refuses it)
              cpu = true;
              wait = ib;
            } else {
              uint32_t node;
              if (keyglob_op(P, B, N, s_cur[d][lane], opw, ia, ic, &node, &keynode)) s_cur[d + 1][lane] = node;
              else wait = ib;
            }
          }
          break;
        case OP_SCOPE_END:
        case OP_POS_END:
          if (A && e.kind) {
            if (op == OP_POS_END) {
              if (e.flags & EF_COND) e.kind = 0;
              else wait = ic;
            } else {
              e.flags |= aux;
              wait = ic;
            }
          }
          break;
        case OP_NEG:
          if (A && kv_lookup_op<ELEM>(N, s_cur[d][lane], ia, aux, rl) != ABSENT) raise(E_NEG, ib, ABSENT, ic);
          break;
        case OP_STAR:
          if (A) {
            const uint32_t v = s_cur[d + 1][lane];
            if (v == ABSENT || node_type(N[v].kt) == NT_NULL) raise(E_STAR, ib, ABSENT, ic);
          }
          break;
        case OP_LEAF:
          if (A) {
            const uint32_t v = s_cur[d][lane];
            Node vn{NT_NULL, 0, 0, 0};
            if (v != ABSENT) vn = N[v];
            const uint32_t vt = node_type(vn.kt);
            bool ok;
            if (vt == NT_ARR) {
              ok = true;
              for (uint32_t k = 0; k < vn.b && ok; k++) {
                if constexpr (ELEM) cpu |= kv_int_unsafe(B, N[kv_nix<ELEM>(vn.a + k, rl)], aux & 1u);
                ok = pred_node(P, B, N, ia, kv_nix<ELEM>(vn.a + k, rl));
              }
            } else {
              if constexpr (ELEM) cpu |= kv_int_unsafe(B, vn, aux & 1u);
              ok = pred_eval(P, B, ia, vt, vn);
            }
            if (!ok) raise(E_VALUE, ib, v, ic);
          }
          break;
        case OP_VLEAF:  // the resource's substituted pattern value (kvvars.cpp): batch predicate table
          if (A) {
            if constexpr (ELEM && VARS) {  // the element's substituted pattern value
              const uint32_t v = s_cur[d][lane];
              const uint32_t dp = vrow[(size_t)ia * vstride + ve];
              const bool sens = (ityp[dp >> 5] >> (dp & 31u)) & 1u;
              Node vn{NT_NULL, 0, 0, 0};
              if (v != ABSENT) vn = N[v];
              const uint32_t vt = node_type(vn.kt);
              bool ok;
              if (vt == NT_ARR) {
                ok = true;
                for (uint32_t k = 0; k < vn.b && ok; k++) {
                  cpu |= kv_int_unsafe(B, N[kv_nix<true>(vn.a + k, rl)], sens);
                  ok = pred_node(*B.dps, B, N, dp, kv_nix<true>(vn.a + k, rl));
                }
              } else {
                cpu |= kv_int_unsafe(B, vn, sens);
                ok = pred_eval(*B.dps, B, dp, vt, vn);
              }
              if (!ok) raise(E_VALUE, ib, v, ic);
            } else if constexpr (ELEM) {  // (no variables in this launch's patterns: kvforeach.h FeVarTables)
              cpu = true;
            } else {
              const uint32_t v = s_cur[d][lane];
              const uint32_t dp = B.dleaf[(size_t)ia * n_res + r];
              Node vn{NT_NULL, 0, 0, 0};
              if (v != ABSENT) vn = N[v];
              const uint32_t vt = node_type(vn.kt);
              bool ok;
              if (vt == NT_ARR) {
                ok = true;
                for (uint32_t k = 0; k < vn.b && ok; k++) ok = pred_node(*B.dps, B, N, dp, ni(vn.a + k));
              } else {
                ok = pred_eval(*B.dps, B, dp, vt, vn);
              }
              if (!ok) raise(E_VALUE, ib, v, ic);
            }
          }
          break;
        case OP_RAISE:
          if (A) raise(ib, ia, s_cur[d][lane], ic);
          break;
        case OP_EXISTCHK:
          if (A) {
            const uint32_t v = s_cur[d][lane];
            if (v == ABSENT || node_type(N[v].kt) != NT_ARR) raise(E_EXIST_RESTYPE, ia, v, ic);
          }
          break;
        case OP_LENCHK:
          if (A && N[s_cur[d][lane]].b < ia) raise(E_LEN, ib, s_cur[d][lane], ic);
          break;
        case OP_INDEX:
          if (A) s_cur[d + 1][lane] = kv_nix<ELEM>(N[s_cur[d][lane]].a + ia, rl);
          break;
        case OP_LOOP_BEGIN:
        case OP_EXIST_BEGIN: {
          if (A) {
            const Node an = N[s_cur[d][lane]];
            s_lfirst[aux][lane] = an.a;
            s_llen[aux][lane] = an.b;
            if (an.b == 0) {
              if (op == OP_LOOP_BEGIN) wait = ia + 1;
              else raise(E_EXIST_FAIL, ib, s_cur[d][lane], ic);
            } else {
              s_cur[d + 1][lane] = kv_nix<ELEM>(an.a, rl);
            }
          }
          if (lane % 64 == 0) s_li[wv][aux] = 0;
          break;
        }
        case OP_LOOP_END:
        case OP_EXIST_END: {
          bool cont = false;
          if (A) {
            if (op == OP_LOOP_END) {
              if (e.kind) {
                if (e.flags & EF_COND) { e.kind = 0; cont = true; }
                else wait = ic;
              } else {
                cont = true;
              }
            } else {
              if (e.kind) { e.kind = 0; cont = true; }  // element failed: try the next one
              else wait = pc + 1;                       // found
            }
            if (cont) {
              const uint32_t i = s_li[wv][aux] + 1;
              if (i < s_llen[aux][lane]) {
                s_cur[d + 1][lane] = kv_nix<ELEM>(s_lfirst[aux][lane] + i, rl);
              } else {
                cont = false;
                if (op == OP_LOOP_END) wait = pc + 1;
                else raise(E_EXIST_FAIL, ib, s_cur[d][lane], ic);
              }
            }
          }
          if (__ballot(cont)) {
            if (lane % 64 == 0) s_li[wv][aux] += 1;
            next = ia + 1;
          }
          break;
        }
        case OP_ALT_BEGIN:
          if (A) { e.kind = 0; e.flags = 0; areg = 0; apres = 0; }
          break;
        case OP_ALT_END:
          if (A) {
            if (e.kind == 0) { st = ST_PASS; wait = KV_SENT; }
            else if (e.kind == E_CPU) { st = ST_CPU; wait = KV_SENT; }
            else if (ib) { st = ST_FAIL; wait = KV_SENT; }
            else { e.kind = 0; e.flags = 0; areg = 0; apres = 0; }
          }
          break;
        case OP_DONE:
          if (A) {
            if (e.kind == 0) st = ST_PASS;
            else if (e.kind == E_CPU) st = ST_CPU;
            else if (e.flags & (EF_COND | EF_GLOBAL)) st = ST_SKIP;
            else if (areg & ~apres) st = ST_ERROR;
            else if (e.kind == E_LEN) st = ST_ERROR;
            else st = ST_FAIL;
            wait = KV_SENT;
          }
          next = KV_SENT;
          break;
        default:
          break;
      }
      if (next == KV_SENT) break;
      pc = next;
    }
  }
}

// The gate and the element's node of element e of foreach set s, whose list's path is steps
// [c0, c0 + cn) of `chain` (FePatTables::chain): one copy for kv_fe_pat_lane and kv_fe_any_lane.
// valid: e is below the list's element count. Returns 0 with *run set where the walk may start
// at *root, else the element's code with *run clear (the lane goes through the walk parked):
//  1. the entry gate (kv_cond_fold<false>): not met ST_SKIP, undecided ST_CPU;
//  2. the element's node: from the resource's root along the list's path (a slot or key-id lookup
//     per field, child k per index); the node the path ends in is the list and the element its
//     child `ord`, or a single map, the one element itself (the one-element rule of evaluateList;
//     behind a field step its trie node carries the element node's keys, kvcompile.cpp). Anything
//     else, a list behind an index step included, is ST_CPU.
// *res / *ord: the element's store resource and its index in its list (0xFFFFFFFF / 0 for a lane
// that is not valid); *rl: the resource's lane in its rows.
__device__ __forceinline__ uint32_t kv_fe_elem_root(const FeTables& T, const uint32_t* __restrict__ chain, const DevBatch& B,
                                                    const Node* __restrict__ N, uint32_t s, uint32_t c0, uint32_t cn,
                                                    uint32_t e, bool valid, uint32_t n_res, uint32_t* res_o, uint32_t* ord_o,
                                                    uint32_t* rl_o, uint32_t* root_o, bool* run_o) {
  const uint32_t* L = T.lists + 4u * T.sets[4u * s];
  const uint32_t n_el = L[1], el0 = L[3];
  uint32_t res = 0xFFFFFFFFu, ord = 0, code = ST_SKIP, rl = 0, root = ABSENT;
  bool run = false;
  if (valid) {
    res = T.el_res[el0 + e];
    ord = T.el_ord[el0 + e];
    code = res < n_res ? 0u : (uint32_t)ST_CPU;
    if (!code && T.sets[4u * s + 1u]) {
      CondBlocks G = T.gate;
      G.outc += L[0];
      code = kv_gate_status(kv_cond_fold<false>(G, s, n_el, e));
    }
    if (!code) {
      rl = res & (KV_LANES - 1u);
      uint32_t node = B.res[res].root * KV_LANES + rl;
      uint32_t last = FE_STEP_SLOT;
      for (uint32_t k = 0; k < cn && node != ABSENT; k++) {
        const uint32_t kind = chain[2u * (c0 + k)], val = chain[2u * (c0 + k) + 1u];
        last = kind;
        if (kind == FE_STEP_INDEX) {
          const Node n = N[node];
          int64_t i = (int32_t)val;
          if (i < 0) i += n.b;
          node = node_type(n.kt) == NT_ARR && i >= 0 && i < (int64_t)n.b ? kv_nix<true>(n.a + (uint32_t)i, rl) : ABSENT;
        } else {
          node = kv_lookup_op<true>(N, node, val, kind == FE_STEP_SCAN ? AUX_SCAN : 0u, rl);
        }
      }
      if (node != ABSENT) {
        const Node n = N[node];
        // a single map is the one element (behind a field step the compiler gave the field's trie
        // node the element node's keys); a list behind an index step has its elements elsewhere
        if (node_type(n.kt) == NT_MAP) root = ord == 0u ? node : ABSENT;
        else if (last != FE_STEP_INDEX && node_type(n.kt) == NT_ARR && ord < n.b) root = kv_nix<true>(n.a + ord, rl);
      }
      run = root != ABSENT && node_type(N[root].kt) == NT_MAP;
      if (!run) code = ST_CPU;
    }
  }
  *res_o = res;
  *ord_o = ord;
  *rl_o = rl;
  *root_o = root;
  *run_o = run;
  return code;
}

// One lane of kv_foreach_pat_kernel (shared with the host harness): element e of the list of
// pattern set p (valid: e is below the list's element count; the other lanes go through the walk
// parked). Returns the element's code and, for ST_FAIL / ST_ERROR, the 8-byte record words in *w;
// *res / *ord: the element's store resource and its index in its list (0xFFFFFFFF / 0 for a lane
// that is not valid). Needs kvblocks.h and kvforeach.h.
//  1. 2. the entry gate and the element's node (kv_fe_elem_root);
//  3. the pattern walk with that node as the root; ST_CPU when the int64 / float64 typing of a
//     number could change the verdict (above) or the record does not fit 8 bytes (which includes
//     the stale counter of a finished loop, below).
// VARS (V: the launch's FeVarTables): between 2. and 3. the substitution verdict of the set's
// strings on the element (kv_fe_subst; the gate's SKIP wins): an element it decides is ST_ERROR
// with a zero record, or ST_CPU, and goes through the walk parked.
template <bool VARS = false>
__device__ __forceinline__ uint32_t kv_fe_pat_lane(const FeTables& T, const FePatTables& Q, const DevPS& P,
                                                   const DevBatch& B, const Node* __restrict__ N, uint32_t p, uint32_t e,
                                                   bool valid, uint32_t n_res, uint32_t (*s_cur)[KV_WG],
                                                   uint32_t (*s_lfirst)[KV_WG], uint32_t (*s_llen)[KV_WG],
                                                   uint32_t (*s_li)[KV_MAXL], uint32_t* res_o, uint32_t* ord_o, uint2* w,
                                                   const FeVarTables* V = nullptr) {
  const uint32_t* PT = Q.pats + 4u * p;
  const uint32_t s = uni(PT[0]);
  uint32_t res, ord, rl, root;
  bool run;
  uint32_t code = kv_fe_elem_root(T, Q.chain, B, N, s, uni(PT[2]), uni(PT[3]), e, valid, n_res, &res, &ord, &rl, &root, &run);
  if constexpr (VARS) {
    const uint32_t* L = T.lists + 4u * T.sets[4u * s];
    w->x = w->y = 0u;
    if (run) {
      const uint32_t sc = kv_fe_subst(T, *V, L, uni(V->runs[2u * p]), uni(V->runs[2u * p + 1u]), e);
      if (sc) {
        code = sc;
        run = false;
      }
    }
  }
  // the wave's loop counters start at zero: an error raised outside a loop records them, and
  // what an earlier program (or kernel) left there must not make the record look too wide.
  // Within one program a finished loop leaves its last index in its counter, and a later error
  // records it although its path needs none: after a level-3 loop (i3 != 0) or a level-0 loop of
  // 1024 iterations or more the record packs as wide and the element is ST_CPU. Conservative.
  if ((threadIdx.x & 63u) == 0u)
    for (uint32_t k = 0; k < KV_MAXL; k++) s_li[threadIdx.x >> 6][k] = 0u;
  uint32_t st = ST_CPU;
  EState es{0, 0, 0, ABSENT, ABSENT, 0, 0, 0, 0};
  bool cpu = false;
  if constexpr (VARS) {
    const uint32_t* L = T.lists + 4u * T.sets[4u * s];
    kv_walk<true, true>(P, B, N, PT + 1, root, run, res, n_res, rl, s_cur, s_lfirst, s_llen, s_li, st, es, cpu,
                        T.deny.outc + L[0], L[1], e, V->ityp);
  } else
    kv_walk<true>(P, B, N, PT + 1, root, run, res, n_res, rl, s_cur, s_lfirst, s_llen, s_li, st, es, cpu);
  if (run) {
    code = cpu ? (uint32_t)ST_CPU : st;
    if (code == ST_FAIL || code == ST_ERROR) {
      *w = err8_pack(es.kind, es.flags, es.pn, es.key, es.i0, es.i1, es.i2, es.i3, rl);
      if (w->x & ERR8_WIDE) code = ST_CPU;
    }
  }
  *res_o = res;
  *ord_o = ord;
  return code;
}

// One lane of kv_foreach_any_kernel (KV_COMPILE_FOREACH_ANYPATTERN; shared with the host harness):
// element e of the list of any set a, after the gate and the node lookup of kv_fe_elem_root. The
// set's alternatives are tried in order as validate() does (validation.go:447-489): each is a
// plain pattern program walked with the element as the root, for the lanes still undecided. The
// alternative count is the same for the whole launch row, and the walk holds wave operations, so
// every lane goes through every call: decided lanes, lanes past the list's end and lanes without
// an element node go parked, and a parked lane's `cpu` and `st` are not read. Per alternative of
// a running lane: the typing guard or ST_CPU makes the element ST_CPU; ST_PASS makes it ST_PASS
// (the later alternatives are not evaluated, so their guard does not count); otherwise (FAIL /
// ERROR / SKIP of that alternative: each is a PatternError the message names) its 8-byte record
// goes to rec[k * stride] and its status into bits [4k, 4k + 4) of the code word; a record that
// does not fit 8 bytes makes the element ST_CPU. A lane undecided after the last alternative is
// ST_FAIL. The wave's loop counters are cleared before every alternative: a finished loop of
// alternative k leaves its last index there, and an error of alternative k + 1 outside any loop
// would record it (a wrong path, or a record that looks wide).
// VARS (V: the launch's FeVarTables): the reference substitutes the whole anyPattern list before
// the first alternative is tried, so the verdict of every alternative's strings (kv_fe_subst over
// the set's run, alternative 0's strings first) comes after the gate and before the loop: an
// element it decides is ST_ERROR or ST_CPU whatever alternative 0 would say.
template <bool VARS = false>
__device__ __forceinline__ uint32_t kv_fe_any_lane(const FeTables& T, const FeAnyTables& A, const DevPS& P,
                                                   const DevBatch& B, const Node* __restrict__ N, uint32_t a, uint32_t e,
                                                   bool valid, uint32_t n_res, uint32_t (*s_cur)[KV_WG],
                                                   uint32_t (*s_lfirst)[KV_WG], uint32_t (*s_llen)[KV_WG],
                                                   uint32_t (*s_li)[KV_MAXL], uint32_t* res_o, uint32_t* ord_o, uint32_t* cw_o,
                                                   uint2* __restrict__ rec, size_t stride,
                                                   const FeVarTables* V = nullptr) {
  const uint32_t* AT = A.anys + 8u * a;
  const uint32_t s = uni(AT[0]), a0 = uni(AT[1]), na = uni(AT[2]);
  uint32_t res, ord, rl, root;
  bool open;  // the lane is still undecided
  uint32_t code = kv_fe_elem_root(T, A.chain, B, N, s, uni(AT[3]), uni(AT[4]), e, valid, n_res, &res, &ord, &rl, &root, &open);
  if constexpr (VARS) {
    const uint32_t* L = T.lists + 4u * T.sets[4u * s];
    if (open) {
      const uint32_t sc = kv_fe_subst(T, *V, L, uni(V->runs[2u * a]), uni(V->runs[2u * a + 1u]), e);
      if (sc) {
        code = sc;
        open = false;
      }
    }
  }
  uint32_t cw = 0;
  for (uint32_t k = 0; k < na; k++) {
    if ((threadIdx.x & 63u) == 0u)
      for (uint32_t j = 0; j < KV_MAXL; j++) s_li[threadIdx.x >> 6][j] = 0u;
    uint32_t st = ST_CPU;
    EState es{0, 0, 0, ABSENT, ABSENT, 0, 0, 0, 0};
    bool cpu = false;
    if constexpr (VARS) {
      const uint32_t* L = T.lists + 4u * T.sets[4u * s];
      kv_walk<true, true>(P, B, N, A.alts + a0 + k, root, open, res, n_res, rl, s_cur, s_lfirst, s_llen, s_li, st, es, cpu,
                          T.deny.outc + L[0], L[1], e, V->ityp);
    } else
      kv_walk<true>(P, B, N, A.alts + a0 + k, root, open, res, n_res, rl, s_cur, s_lfirst, s_llen, s_li, st, es, cpu);
    if (open) {
      if (cpu || st == ST_CPU) {
        code = ST_CPU;
        open = false;
      } else if (st == ST_PASS) {
        code = ST_PASS;
        open = false;
      } else {
        const uint2 w = err8_pack(es.kind, es.flags, es.pn, es.key, es.i0, es.i1, es.i2, es.i3, rl);
        if (w.x & ERR8_WIDE) {
          code = ST_CPU;
          open = false;
        } else {
          rec[k * stride] = w;
          cw |= st << (4u * k);
        }
      }
    }
  }
  if (open) code = ST_FAIL;
  *res_o = res;
  *ord_o = ord;
  *cw_o = code == ST_FAIL ? cw : 0u;
  return code;
}
