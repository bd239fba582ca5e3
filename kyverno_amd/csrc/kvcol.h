// Path columns (kvdevtypes.h ColDesc / ColFam): built once per batch and device from the node
// rows, read by the specialized kernels in place of their row walks (kvjitgen.cpp hoist). Device
// functions over the kvdevfn.h helpers: the kv_pcol_* kernels (kvkernel.hip) and the host
// emulator (tools/kvemu/mtab.cpp) run these bodies. Include after kvdevfn.h.
//
// A column cell is what the specialized kernels' row walk leaves in its hoisted node
// (kvjitgen.cpp hoist): the node at the path, or all zero when a step finds no node (a missing
// key, a non-map parent, a slot past the map's slots); the present cells carry
// KV_COL_PRESENT in kt (their key is dropped: the walk never reads a hoisted node's key) and
// in c the node's own index when it is a map (the cursor of a wildcard-key lookup) or the
// word offset of its element rows when it holds a family's array. A narrow column keeps one
// word of it (kvdevfn.h kv_narrow_cell).
#pragma once

// the node one step below n (held in cell *idx, ABSENT: none)
KV_FN Node col_step(const Node* __restrict__ N, const Node& n, uint32_t step, uint32_t* idx) {
  const Node z{0u, 0u, 0u, 0u};
  if (*idx == ABSENT || node_type(n.kt) != NT_MAP) {
    *idx = ABSENT;
    return z;
  }
  if (step & KV_COL_SCAN) {  // keep-all map (labels / annotations): the child with that key
    const uint32_t key = step & ~KV_COL_SCAN;
    for (uint32_t q = 0; q < n.b; q++) {
      const uint32_t c = ni(n.a + q);
      const Node t = N[c];
      if (node_key(t.kt) == key) {
        *idx = c;
        return t;
      }
    }
    *idx = ABSENT;
    return z;
  }
  if (step >= n.b) {  // slot-addressed map: slot `step`, NT_ABSENT when the resource lacks it
    *idx = ABSENT;
    return z;
  }
  const uint32_t c = ni(n.a + step);
  const Node t = N[c];
  if (node_type(t.kt) == NT_ABSENT) {
    *idx = ABSENT;
    return z;
  }
  *idx = c;
  return t;
}

// the node at column path d below cell idx (ABSENT: none), its cell in *out
KV_FN Node col_walk(const Node* __restrict__ N, uint32_t idx, const ColDesc& d, uint32_t* out) {
  Node n{0u, 0u, 0u, 0u};
  if (idx != ABSENT) n = N[idx];
  for (uint32_t s = 0; s < d.nsteps && s < KV_COL_MAXD; s++) n = col_step(N, n, d.steps[s], &idx);
  *out = idx;
  return n;
}

KV_FN Node col_cell(const Node& n, uint32_t idx, uint32_t arr_c) {
  if (idx == ABSENT) return Node{0u, 0u, 0u, 0u};
  const uint32_t t = node_type(n.kt);
  return Node{t | KV_COL_PRESENT, n.a, n.b, t == NT_MAP ? idx : t == NT_ARR ? arr_c : n.c};
}

KV_FN uint64_t col_fam_off(const ColFam& F) { return (uint64_t)F.off_lo | (uint64_t)F.off_hi << 32; }
// words of one row of family F: [wide (kt, a, c) x nw x 64][b x nb x 64][narrow x nn x 64]
KV_FN uint32_t col_row_words(const ColFam& F) { return (3u * F.nw + F.nb + F.nn) * KV_LANES; }

// lane `lane`'s cell of column d in the row of family F that starts at word `row` of the pool
// (idx: the node's index)
KV_FN void col_put(uint32_t* __restrict__ pool, uint64_t row, const ColFam& F, const ColDesc& d, uint32_t lane,
                   const Node& n, uint32_t idx) {
  if (d.fmt == KV_COLF_NARROW) {
    pool[row + (size_t)(3u * F.nw + F.nb + d.pos) * KV_LANES + lane] = kv_narrow_cell(n.kt, n.a, idx);
    return;
  }
  uint32_t* __restrict__ w = pool + row + (size_t)d.pos * (3u * KV_LANES) + 3u * lane;
  w[0] = n.kt;
  w[1] = n.a;
  w[2] = n.c;
  if (d.fmt == KV_COLF_WIDEB) pool[row + (size_t)(3u * F.nw + d.bpos) * KV_LANES + lane] = n.b;
}
// a wide cell with its b (a family array's)
KV_FN Node col_get(const uint32_t* __restrict__ pool, uint64_t row, const ColFam& F, const ColDesc& d, uint32_t lane) {
  const uint32_t* __restrict__ w = pool + row + (size_t)d.pos * (3u * KV_LANES) + 3u * lane;
  return Node{w[0], w[1], pool[row + (size_t)(3u * F.nw + d.bpos) * KV_LANES + lane], w[2]};
}

// lane r's cell of the root-path array that family F (not a nested one) belongs to, from the
// built rows of family 0: a wide cell with its b, c = the word offset of the lane's element rows
KV_FN Node col_root_arr(const uint32_t* __restrict__ pool, const ColDesc* cols, const ColFam* fams, const ColFam& F,
                        uint32_t r) {
  return col_get(pool, (uint64_t)(r >> 6) * col_row_words(fams[0]), fams[0], cols[F.arr_col], r & (KV_LANES - 1));
}
KV_FN bool col_is_arr(const Node& a) { return a.kt != 0u && node_type(a.kt) == NT_ARR; }

// element rows lane r needs in family f, not a nested one (its array's element count; 0 without
// an array)
KV_FN uint32_t col_rows(const DevBatch& B, const ColDesc* cols, const ColFam* fams, uint32_t f, uint32_t r) {
  if (r >= B.n_res) return 0u;
  uint32_t idx;
  const Node n = col_walk(B.nodes, ni(B.res[r].root), cols[fams[f].arr_col], &idx);
  return idx != ABSENT && node_type(n.kt) == NT_ARR ? n.b : 0u;
}

// Rows of a nested family f, from the node rows: col_nested_parent is lane r's array of f's
// parent family (its node; all zero without one), col_rows_nested the rows the lane needs below
// element i of that array (the nested array's element count; 0 without that element or without
// an array in it). The rows of parent row (wave group, i) are the most any of the group's lanes
// needs.
KV_FN Node col_nested_parent(const DevBatch& B, const ColDesc* cols, const ColFam* fams, uint32_t f, uint32_t r) {
  const Node z{0u, 0u, 0u, 0u};
  if (r >= B.n_res) return z;
  uint32_t idx;
  const Node a = col_walk(B.nodes, ni(B.res[r].root), cols[fams[fams[f].parent].arr_col], &idx);
  return idx != ABSENT && node_type(a.kt) == NT_ARR ? a : z;
}
KV_FN uint32_t col_rows_nested(const DevBatch& B, const ColDesc* cols, const ColFam* fams, uint32_t f, const Node& a,
                               uint32_t i) {
  if (i >= a.b) return 0u;
  uint32_t idx;
  const Node n = col_walk(B.nodes, ni(a.a + i), cols[fams[f].arr_col], &idx);
  return idx != ABSENT && node_type(n.kt) == NT_ARR ? n.b : 0u;
}

// cell of family-0 column `c` for lane r (r >= n_res: the zero cell), written into the pool
KV_FN void col_build_root(const DevBatch& B, const ColDesc* cols, const ColFam* fams, uint32_t c, uint32_t r,
                          uint32_t* __restrict__ pool) {
  const ColDesc& d = cols[c];
  Node cell{0u, 0u, 0u, 0u};
  uint32_t idx = ABSENT;
  if (r < B.n_res) {
    const Node n = col_walk(B.nodes, ni(B.res[r].root), d, &idx);
    uint32_t arr_c = 0u;
    if (d.arr_fam) {  // a family array: the word offset of this wave group's element rows
      const ColFam& F = fams[d.arr_fam];
      arr_c = (uint32_t)(col_fam_off(F) + (uint64_t)F.erow[r >> 6] * col_row_words(F));
    }
    cell = col_cell(n, idx, arr_c);
  }
  col_put(pool, (uint64_t)(r >> 6) * col_row_words(fams[0]), fams[0], d, r & (KV_LANES - 1), cell, idx);
}

// cell of element column `c` (of a family of a root-path array, whose cell must be built) for
// element i of lane r's array, if it has one; arr_c: for a column that holds a nested family's
// array, the word offset of the nested rows of this parent row (col_nested_off). Returns the
// element count of an array at the cell (0: none): the rows this lane needs in that nested family.
KV_FN uint32_t col_build_elem_at(const DevBatch& B, const ColDesc* cols, const ColFam* fams, uint32_t c, uint32_t r, uint32_t i,
                             uint32_t arr_c, uint32_t* __restrict__ pool) {
  const ColDesc& d = cols[c];
  const ColFam& F = fams[d.fam];
  const Node a = col_root_arr(pool, cols, fams, F, r);
  if (!col_is_arr(a) || i >= a.b) return 0u;
  uint32_t idx;
  const Node n = col_walk(B.nodes, ni(a.a + i), d, &idx);
  col_put(pool, (uint64_t)a.c + (uint64_t)i * col_row_words(F), F, d, r & (KV_LANES - 1), col_cell(n, idx, arr_c), idx);
  return idx != ABSENT && node_type(n.kt) == NT_ARR ? n.b : 0u;
}
// elements lane r has in the array of the family of element column c (built, as above)
KV_FN uint32_t col_elems(const ColDesc* cols, const ColFam* fams, uint32_t c, uint32_t r, const uint32_t* __restrict__ pool) {
  const Node a = col_root_arr(pool, cols, fams, fams[cols[c].fam], r);
  return col_is_arr(a) ? a.b : 0u;
}
// word offset of the rows of nested family N that follow `run` rows of wave group g
KV_FN uint32_t col_nested_off(const ColFam& N, uint32_t g, uint32_t run) {
  return (uint32_t)(col_fam_off(N) + (uint64_t)(N.erow[g] + run) * col_row_words(N));
}

// cells of element column `c` (as col_build_elem_at; not a nested family's array) for every
// element of lane r's family array
KV_FN void col_build_elem(const DevBatch& B, const ColDesc* cols, const ColFam* fams, uint32_t c, uint32_t r,
                          uint32_t* __restrict__ pool) {
  for (uint32_t i = 0, n = col_elems(cols, fams, c, r, pool); i < n; i++) col_build_elem_at(B, cols, fams, c, r, i, 0u, pool);
}

// cells of column `c` of a nested family for every element of every nested array of lane r (the
// parent family's cells of the nested array, wide ones with their b, must be built)
KV_FN void col_build_nested(const DevBatch& B, const ColDesc* cols, const ColFam* fams, uint32_t c, uint32_t r,
                            uint32_t* __restrict__ pool) {
  const ColDesc& d = cols[c];
  const ColFam& F = fams[d.fam];
  const ColFam& P = fams[F.parent];
  const uint32_t lane = r & (KV_LANES - 1);
  const Node a = col_root_arr(pool, cols, fams, P, r);
  if (!col_is_arr(a)) return;
  for (uint32_t i = 0; i < a.b; i++) {
    const Node e = col_get(pool, (uint64_t)a.c + (uint64_t)i * col_row_words(P), P, cols[F.arr_col], lane);
    if (!col_is_arr(e)) continue;
    for (uint32_t k = 0; k < e.b; k++) {
      uint32_t idx;
      const Node n = col_walk(B.nodes, ni(e.a + k), d, &idx);
      col_put(pool, (uint64_t)e.c + (uint64_t)k * col_row_words(F), F, d, lane, col_cell(n, idx, 0u), idx);
    }
  }
}
