// Host plan of the sparse negative-semidefiniteness check (cert_chol.hpp): symbolic elimination of the clique pattern in its stored
// order with the affine index `a` = n - 1 last.  Integer work only, no GPU.
//
// The pattern of Z lives on the cliques, and their natural order (layers, then x_K, then a) is a perfect elimination order for the
// Single and Path cliques (no fill) and fills the Double cliques up to Single's pattern.  The plan is what a multifrontal Cholesky of
// N = -Z needs: supernodes (consecutive column ranges of equal structure - the reduced layers on the network patterns), the row list
// below each diagonal block (fill included), the elimination forest, the gather list from the NE-vector into each front and the
// placement of every update matrix in a per-candidate scratch.  The row of `a` is put into EVERY front as its last row, so the forward
// solve of z_xa rides along and what is left of (a, a) at the end is the Schur complement.
#pragma once
#include <algorithm>
#include <cstdint>
#include <iterator>
#include <utility>
#include <vector>

#include "setup.hpp"

namespace nnsdp {

static constexpr int kCertFrontMax = 128;    // largest front (supernode columns + rows below, a included): a full square in LDS

struct CertPlan {
  int n = 0, n_super = 0, max_front = 0, e_aa = -1;
  long long fill = 0;                 // entries of the factor's structure (below the diagonal, columns 0 .. n-2) outside the pattern
  bool supported = false;             // max_front <= kCertFrontMax
  std::vector<int> col_start;         // n_super + 1; col_start[n_super] = n - 1 (a is no supernode)
  std::vector<int> row_ptr, row_idx;  // rows below the diagonal block of supernode s, ascending; the last one is a
  std::vector<int> parent;            // supernode holding the first row of the list; -1: the list is {a} (a root of the forest)
  std::vector<int> rel;               // (aligned with row_idx) position of that row in the parent's front; roots: 0
  std::vector<int> child_ptr, child_idx;   // children of every supernode, ascending
  std::vector<int> roots;             // ascending
  std::vector<int> gat_ptr, gat_pos, gat_ent;   // per supernode: front position (row << 8 | column, row >= column) <- pattern entry
  std::vector<long long> upd_off;     // where supernode s leaves its update matrix (rows x rows, lower, column-major) in the scratch
  long long scratch = 0;              // doubles of scratch per candidate
  int rows(int s) const { return row_ptr[s + 1] - row_ptr[s]; }
  int cols(int s) const { return col_start[s + 1] - col_start[s]; }
  int front(int s) const { return cols(s) + rows(s); }
};

inline CertPlan make_cert_plan(const Pattern& pat) {
  CertPlan pl;
  const int n = pat.n, a = n - 1;
  pl.n = n;
  if (n < 1) return pl;
  pl.e_aa = pat.pos(a, a);
  // column structures of the factor (elimination game, columns 0 .. n-2; a is never eliminated and is forced into every column)
  std::vector<std::vector<int>> st(std::max(a, 0));
  std::vector<std::vector<int>> kids(std::max(a, 0));
  std::vector<int> par(std::max(a, 0), -1), tmp;
  for (int j = 0; j < a; ++j) {
    std::vector<int>& s = st[j];
    for (int i = j + 1; i < n; ++i)
      if (pat.pos(i, j) >= 0) s.push_back(i);
    long long in_pattern = (long long)s.size();
    if (s.empty() || s.back() != a) s.push_back(a);
    for (int c : kids[j]) {
      tmp.clear();
      std::set_union(s.begin(), s.end(), st[c].begin() + 1, st[c].end(), std::back_inserter(tmp));   // st[c][0] == j
      s.swap(tmp);
    }
    pl.fill += (long long)s.size() - in_pattern;
    if (s[0] != a) { par[j] = s[0]; kids[s[0]].push_back(j); }
  }
  // supernodes: column j + 1 joins column j when struct(j) = {j + 1} + struct(j + 1)
  pl.col_start.push_back(0);
  for (int j = 0; j + 1 < a; ++j)
    if (!(par[j] == j + 1 && st[j].size() == st[j + 1].size() + 1)) pl.col_start.push_back(j + 1);
  if (a > 0) pl.col_start.push_back(a);
  pl.n_super = (int)pl.col_start.size() - 1;
  std::vector<int> super_of(n, -1);
  for (int s = 0; s < pl.n_super; ++s)
    for (int j = pl.col_start[s]; j < pl.col_start[s + 1]; ++j) super_of[j] = s;
  pl.row_ptr.assign(1, 0);
  pl.parent.assign(pl.n_super, -1);
  for (int s = 0; s < pl.n_super; ++s) {
    const std::vector<int>& last = st[pl.col_start[s + 1] - 1];
    pl.row_idx.insert(pl.row_idx.end(), last.begin(), last.end());
    pl.row_ptr.push_back((int)pl.row_idx.size());
    if (last[0] != a) pl.parent[s] = super_of[last[0]];
    pl.max_front = std::max(pl.max_front, pl.front(s));
  }
  if (pl.n_super == 0) pl.max_front = 1;
  pl.supported = pl.max_front <= kCertFrontMax;
  // children, roots, relative positions
  pl.child_ptr.assign(pl.n_super + 1, 0);
  for (int s = 0; s < pl.n_super; ++s) {
    if (pl.parent[s] >= 0) pl.child_ptr[pl.parent[s] + 1]++;
    else pl.roots.push_back(s);
  }
  for (int s = 0; s < pl.n_super; ++s) pl.child_ptr[s + 1] += pl.child_ptr[s];
  pl.child_idx.resize(pl.child_ptr[pl.n_super]);
  {
    std::vector<int> at(pl.child_ptr.begin(), pl.child_ptr.end() - 1);
    for (int s = 0; s < pl.n_super; ++s)
      if (pl.parent[s] >= 0) pl.child_idx[at[pl.parent[s]]++] = s;
  }
  std::vector<int> where(n, -1);
  auto mark_front = [&](int s, bool set) {
    int q = 0;
    for (int j = pl.col_start[s]; j < pl.col_start[s + 1]; ++j) where[j] = set ? q++ : -1;
    for (int t = pl.row_ptr[s]; t < pl.row_ptr[s + 1]; ++t) where[pl.row_idx[t]] = set ? q++ : -1;
  };
  pl.rel.assign(pl.row_idx.size(), 0);
  pl.gat_ptr.assign(1, 0);
  for (int s = 0; s < pl.n_super; ++s) {
    mark_front(s, true);
    for (int t = pl.child_ptr[s]; t < pl.child_ptr[s + 1]; ++t) {
      const int c = pl.child_idx[t];
      for (int q = pl.row_ptr[c]; q < pl.row_ptr[c + 1]; ++q) pl.rel[q] = where[pl.row_idx[q]];   // (a subset of this front: >= 0)
    }
    for (int j = pl.col_start[s]; j < pl.col_start[s + 1]; ++j)
      for (int i = j; i < n; ++i) {
        const int e = pat.pos(i, j);
        if (e < 0) continue;
        pl.gat_pos.push_back(where[i] << 8 | where[j]);
        pl.gat_ent.push_back(e);
      }
    pl.gat_ptr.push_back((int)pl.gat_ent.size());
    mark_front(s, false);
  }
  // scratch placement: the update matrix of s lives from the end of s to the assembly of its parent; first fit over the live ones
  pl.upd_off.assign(pl.n_super, 0);
  std::vector<std::pair<long long, long long>> live;    // (offset, size), sorted by offset
  std::vector<long long> size_of(pl.n_super);
  for (int s = 0; s < pl.n_super; ++s) {
    for (int t = pl.child_ptr[s]; t < pl.child_ptr[s + 1]; ++t) {
      const int c = pl.child_idx[t];
      if (pl.parent[c] < 0) continue;
      live.erase(std::find(live.begin(), live.end(), std::make_pair(pl.upd_off[c], size_of[c])));
    }
    size_of[s] = (long long)pl.rows(s) * pl.rows(s);
    long long off = 0;
    size_t at = 0;
    for (; at < live.size(); ++at) {
      if (live[at].first - off >= size_of[s]) break;
      off = live[at].first + live[at].second;
    }
    live.insert(live.begin() + at, std::make_pair(off, size_of[s]));     // (roots stay live: their 1 x 1 is summed at the end)
    pl.upd_off[s] = off;
    pl.scratch = std::max(pl.scratch, off + size_of[s]);
  }
  pl.scratch = std::max<long long>(pl.scratch, 1);
  return pl;
}

}  // namespace nnsdp
