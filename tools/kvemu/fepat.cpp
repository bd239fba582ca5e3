// kvemu: host build of the pattern walk (kvwalk.h: the interpreter loop of kv_validate_kernel and
// the per-lane bodies of kv_foreach_pat_kernel and kv_foreach_any_kernel) as a one-lane wave, with the prelude the specialized
// kernels see: the pattern sets' rows of the deny plane (KV_COMPILE_FOREACH_PATTERN), element by
// element, reduced as kv_foreach_elem_kernel's keys are and finished as kv_foreach_fin_kernel does.
#include "shim.h"
#include "../../build/kvgpu/kvjit_prelude.h"
#include "../../kyverno_amd/csrc/kvblocks.h"
#include "../../kyverno_amd/csrc/kvforeach.h"
#include "../../kyverno_amd/csrc/kvwalk.h"

#include <algorithm>
#include <vector>

// fe_st[set][res] of every pattern set of Q (rows `set` of fe_st, n_res bytes each). The last
// n_vpats pattern sets hold variable strings (KV_COMPILE_FOREACH_PATVARS): as launch_foreach runs
// them, through the VARS instantiation over the tables from the first of them on (V: the runs of
// every pattern set, then of every any set)
extern "C" void kvemu_foreach_pat(const FeTables* T, const FePatTables* Q, const DevPS* P, const DevBatch* B,
                                  uint32_t n_res, uint8_t* fe_st, const FeVarTables* V, uint32_t n_vpats) {
  static thread_local uint32_t s_cur[KV_MAXD][KV_WG], s_lfirst[KV_MAXL][KV_WG], s_llen[KV_MAXL][KV_WG],
      s_li[KV_WG / 64][KV_MAXL];
  threadIdx.x = 0;
  std::vector<uint32_t> key(n_res);
  for (uint32_t p = 0; p < Q->n_pats; p++) {
    const uint32_t s = Q->pats[4u * p], list = T->sets[4u * s];
    const uint32_t n_el = T->lists[4u * list + 1u];
    std::fill(key.begin(), key.end(), FE_KEY_NONE);
    for (uint32_t e = 0; e < n_el; e++) {
      uint32_t res, ord;
      uint2 w{0u, 0u};
      uint32_t code;
      if (p < Q->n_pats - n_vpats) {
        code = kv_fe_pat_lane(*T, *Q, *P, *B, B->nodes, p, e, true, n_res, s_cur, s_lfirst, s_llen, s_li, &res, &ord, &w);
      } else {
        const uint32_t p0 = Q->n_pats - n_vpats;
        FePatTables Q1 = *Q;
        Q1.pats += 4u * p0;
        Q1.n_pats = n_vpats;
        FeVarTables V1 = *V;
        V1.runs += 2u * p0;
        code = kv_fe_pat_lane<true>(*T, Q1, *P, *B, B->nodes, p - p0, e, true, n_res, s_cur, s_lfirst, s_llen, s_li, &res,
                                    &ord, &w, &V1);
      }
      if (res < n_res) key[res] = std::min(key[res], kv_fe_key(code, ord));
    }
    for (uint32_t r = 0; r < n_res; r++)
      fe_st[(size_t)s * n_res + r] = (uint8_t)kv_fe_final(T->lstate[(size_t)list * n_res + r], key[r]);
  }
}

// fe_st[set][res] of every any set of A (KV_COMPILE_FOREACH_ANYPATTERN): the lane body of
// kv_foreach_any_kernel per element, the records of one element at a time
// (the last n_vanys any sets hold variable strings, as above; n_pats: the runs of the pattern sets
// stand in front of the any sets')
extern "C" void kvemu_foreach_any(const FeTables* T, const FeAnyTables* A, const DevPS* P, const DevBatch* B,
                                  uint32_t n_res, uint8_t* fe_st, const FeVarTables* V, uint32_t n_vanys, uint32_t n_pats) {
  static thread_local uint32_t s_cur[KV_MAXD][KV_WG], s_lfirst[KV_MAXL][KV_WG], s_llen[KV_MAXL][KV_WG],
      s_li[KV_WG / 64][KV_MAXL];
  threadIdx.x = 0;
  std::vector<uint32_t> key(n_res);
  for (uint32_t a = 0; a < A->n_anys; a++) {
    const uint32_t s = A->anys[8u * a], list = T->sets[4u * s];
    const uint32_t n_el = T->lists[4u * list + 1u];
    std::fill(key.begin(), key.end(), FE_KEY_NONE);
    for (uint32_t e = 0; e < n_el; e++) {
      uint32_t res, ord, cw;
      uint2 rec[FE_MAX_ALTS];
      uint32_t code;
      if (a < A->n_anys - n_vanys) {
        code = kv_fe_any_lane(*T, *A, *P, *B, B->nodes, a, e, true, n_res, s_cur, s_lfirst, s_llen, s_li, &res, &ord, &cw,
                              rec, 1);
      } else {
        const uint32_t a0 = A->n_anys - n_vanys;
        FeAnyTables A1 = *A;
        A1.anys += 8u * a0;
        A1.n_anys = n_vanys;
        FeVarTables V1 = *V;
        V1.runs += 2u * (n_pats + a0);
        code = kv_fe_any_lane<true>(*T, A1, *P, *B, B->nodes, a - a0, e, true, n_res, s_cur, s_lfirst, s_llen, s_li, &res,
                                    &ord, &cw, rec, 1, &V1);
      }
      if (res < n_res) key[res] = std::min(key[res], kv_fe_key(code, ord));
    }
    for (uint32_t r = 0; r < n_res; r++)
      fe_st[(size_t)s * n_res + r] = (uint8_t)kv_fe_final(T->lstate[(size_t)list * n_res + r], key[r]);
  }
}
