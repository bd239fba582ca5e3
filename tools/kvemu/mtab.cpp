// kvemu: host build of the pass's match-table builder (kvdevfn.h mtab_word, the
// body of kv_mtab_kernel) and of the factored match (fac_cell / mtup_word, the bodies of
// kv_mfac_kernel / kv_mtup_kernel), with the same prelude the specialized kernels see.
#include "shim.h"
#include "../../build/kvgpu/kvjit_prelude.h"
#include "../../kyverno_amd/csrc/kvfac.h"
#include "../../kyverno_amd/csrc/kvcol.h"

#include <algorithm>
#include <stdexcept>
#include <vector>

extern "C" void kvemu_mtab(const DevPS* P, const DevBatch* B, uint32_t words, uint32_t max_entities, uint32_t* ns,
                           uint32_t* an, uint32_t* sl) {
  for (uint32_t y = 0; y < words; y++)
    for (uint32_t e = 0; e < max_entities; e++) mtab_word(*P, *B, y, e, ns, an, sl);
}

extern "C" void kvemu_mfac(const DevPS* P, const DevBatch* B, uint32_t* mtup) {
  for (uint32_t t = 0; t < KV_FAC_TYPES; t++)
    for (uint32_t s = 0; s < P->fac_slots; s++)
      for (uint32_t e = 0, ne = fac_entities(*B, t); e < ne; e++)
        P->fac_tab[P->fac_off[t] + (size_t)s * ne + e] = fac_cell(*P, *B, t, e, s);
  for (uint32_t w = 0; w < P->fac_words; w++)
    for (uint32_t t = 0; t < B->n_tup; t++) mtup[(size_t)w * B->n_tup + t] = mtup_word(*P, *B, t, w);
}

// path columns (as build_pcol in kvapi.cpp, the kv_pcol_* kernels lane by lane): family 0,
// the element rows of every wave group and family (max over the group's lanes, a nested
// family's summed over its parent's rows; exclusive prefix), the families' offsets, then the
// element columns and the nested families' columns; returns the pool
std::vector<uint32_t> kvemu_pcol(const DevBatch* B, const std::vector<ColDesc>& cols, const std::vector<uint32_t>& fam_arr,
                                 const std::vector<uint32_t>& fam_parent, const std::vector<uint32_t>& fam_ncols, const std::vector<uint32_t>& fam_nw,
                                 const std::vector<uint32_t>& fam_nb, const std::vector<uint32_t>& fam_nn,
                                 std::vector<uint32_t>* erow) {
  const uint32_t nf = (uint32_t)fam_ncols.size(), j0 = fam_ncols.at(0);
  const uint32_t groups = (uint32_t)((B->n_res + KV_WG - 1) / KV_WG * (KV_WG / KV_LANES));
  erow->assign((size_t)std::max<uint32_t>(1u, nf - 1) * (groups + 1), 0u);
  std::vector<ColFam> fams(nf);
  for (uint32_t f = 0; f < nf; f++) {
    fams[f].arr_col = fam_arr[f];
    fams[f].parent = fam_parent.at(f);
    fams[f].ncols = fam_ncols[f];
    fams[f].nw = fam_nw.at(f);
    fams[f].nb = fam_nb.at(f);
    fams[f].nn = fam_nn.at(f);
    fams[f].erow = f ? erow->data() + (size_t)(f - 1) * (groups + 1) : nullptr;
  }
  // (a wave's maximum of per-lane values fn(r) of group g)
  auto wave_max = [&](uint32_t g, auto fn) {
    uint32_t m = 0;
    for (uint32_t r = g * KV_LANES; r < (g + 1) * KV_LANES; r++) {
      threadIdx.x = r % KV_WG;
      m = std::max(m, fn(r));
    }
    return m;
  };
  for (int nested = 0; nested < 2; nested++)  // parents first: a nested family counts per parent row
    for (uint32_t f = 1; f < nf; f++) {
      if ((fams[f].parent != 0) != (nested != 0)) continue;
      for (uint32_t g = 0; g < groups; g++) {
        if (!nested) {
          fams[f].erow[g] = wave_max(g, [&](uint32_t r) { return col_rows(*B, cols.data(), fams.data(), f, r); });
          continue;
        }
        for (uint32_t i = 0, n = fams[fams[f].parent].erow[g]; i < n; i++)
          fams[f].erow[g] += wave_max(g, [&](uint32_t r) {
            return col_rows_nested(*B, cols.data(), fams.data(), f, col_nested_parent(*B, cols.data(), fams.data(), f, r), i);
          });
      }
    }
  for (uint32_t f = 1; f < nf; f++) {
    uint32_t* e = fams[f].erow;
    uint32_t run = 0;
    for (uint32_t g = 0; g <= groups; g++) {
      const uint32_t c = g < groups ? e[g] : 0u;
      e[g] = run;
      run += c;
    }
  }
  uint64_t words = (uint64_t)groups * col_row_words(fams[0]);
  for (uint32_t f = 1; f < nf; f++) {
    fams[f].off_lo = (uint32_t)words;
    fams[f].off_hi = (uint32_t)(words >> 32);
    words += (uint64_t)fams[f].erow[groups] * col_row_words(fams[f]);
  }
  if (words >= (1ull << 32)) throw std::runtime_error("kvemu: more than 2^32 column words");
  // (exactly the pool's words: a read past a row's end is out of bounds)
  std::vector<uint32_t> pool(std::max<uint64_t>(words, 1), 0u);
  for (uint32_t level = 0; level < 3; level++)  // (kv_pcol_build_kernel, level by level)
    for (uint32_t c = 0; c < cols.size(); c++) {
      const ColDesc& d = cols[c];
      if (level == 0 ? c >= j0 : c < j0 || (fams[d.fam].parent != 0) != (level == 2)) continue;
      auto lanes = [&](uint32_t g0, uint32_t g1, auto fn) {
        for (uint32_t r = g0 * KV_LANES; r < g1 * KV_LANES; r++) {
          threadIdx.x = r % KV_WG;
          fn(r);
        }
      };
      if (level == 0) lanes(0, groups, [&](uint32_t r) { col_build_root(*B, cols.data(), fams.data(), c, r, pool.data()); });
      else if (level == 2) lanes(0, groups, [&](uint32_t r) { col_build_nested(*B, cols.data(), fams.data(), c, r, pool.data()); });
      else if (!d.arr_fam) lanes(0, groups, [&](uint32_t r) { col_build_elem(*B, cols.data(), fams.data(), c, r, pool.data()); });
      else  // a nested family's array: wave by wave, the nested rows of a parent row after those before it
        for (uint32_t g = 0; g < groups; g++) {
          const uint32_t n = wave_max(g, [&](uint32_t r) { return col_elems(cols.data(), fams.data(), c, r, pool.data()); });
          for (uint32_t i = 0, run = 0; i < n; i++) {
            const uint32_t off = col_nested_off(fams[d.arr_fam], g, run);
            run += wave_max(g, [&](uint32_t r) { return col_build_elem_at(*B, cols.data(), fams.data(), c, r, i, off, pool.data()); });
          }
        }
    }
  return pool;
}
