// eg_structure.h -- the host-built structure of OptimizeEssentialGraph's linear system (the
// arrays EgGraph of eg_kernels.h points to): free vertices, the profile of the 7F x 7F system,
// the assembly targets and the factorisation's column extents. Plain host C++, no HIP calls:
// optimizer_runtime.cpp builds the graph with it, tests/eg_step_check.hip runs the same function.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../../include/slamgpu_optimizer.h"

namespace slamgpu {

struct EgStructure {
  int F = 0;             // free vertices
  int64_t n_blocks = 0;  // blocks of the profile (off[F])
  std::vector<int32_t> fidx;   // [n_kf] free index or -1
  std::vector<int32_t> start;  // [F] first block column of row f
  std::vector<int64_t> off;    // [F + 1] block row f stores blocks start[f] .. f at off[f]
  // assembly targets: the F diagonal blocks, then the off-diagonal blocks in the order edges
  // first touch them; item = edge * 4 + kind (eg_kernels.h)
  std::vector<int32_t> tgt_block, tgt_vertex, tgt_ptr, tgt_items;
  // column extents: rows i > k with start[i] <= k, increasing; ext_base = off[row] - start[row]
  std::vector<int32_t> ext_ptr, ext_rows;
  std::vector<int64_t> ext_base;
};

// Edges must name valid, distinct keyframes (the caller validates).
inline EgStructure eg_build_structure(int n_kf, const uint8_t* fixed,
                                      const slamgpu_sim3_edge* edges, int n_edges) {
  EgStructure s;
  std::vector<int32_t>& fidx = s.fidx;
  fidx.resize(n_kf);
  int F = 0;
  for (int v = 0; v < n_kf; v++) fidx[v] = fixed[v] ? -1 : F++;
  s.F = F;
  std::vector<int32_t>& start = s.start;
  start.resize(F);
  for (int f = 0; f < F; f++) start[f] = f;
  for (int k = 0; k < n_edges; k++) {
    const int a = fidx[edges[k].i], b = fidx[edges[k].j];
    if (a < 0 || b < 0) continue;
    const int hi = std::max(a, b), lo = std::min(a, b);
    start[hi] = std::min(start[hi], lo);
  }
  std::vector<int64_t>& off = s.off;
  off.assign(F + 1, 0);
  for (int f = 0; f < F; f++) off[f + 1] = off[f] + (f - start[f] + 1);
  const int64_t n_blocks = off[F];
  s.n_blocks = n_blocks;
  std::vector<std::vector<int32_t>> items(F);
  std::vector<std::vector<int32_t>> off_items;
  std::vector<int64_t> off_key;  // block of each off-diagonal target
  {
    std::vector<int32_t> blk2t((size_t)n_blocks, -1);
    for (int k = 0; k < n_edges; k++) {
      const int a = fidx[edges[k].i], b = fidx[edges[k].j];
      if (a >= 0) items[a].push_back(4 * k + 0);
      if (b >= 0) items[b].push_back(4 * k + 1);
      if (a >= 0 && b >= 0) {
        const int hi = std::max(a, b), lo = std::min(a, b);
        const int64_t blk = off[hi] + (lo - start[hi]);
        if (blk2t[blk] < 0) {
          blk2t[blk] = (int32_t)off_items.size();
          off_items.emplace_back();
          off_key.push_back(blk);
        }
        off_items[blk2t[blk]].push_back(4 * k + (a > b ? 2 : 3));
      }
    }
  }
  s.tgt_ptr.assign(1, 0);
  for (int f = 0; f < F; f++) {
    s.tgt_block.push_back((int32_t)(off[f] + (f - start[f])));
    s.tgt_vertex.push_back(f);
    s.tgt_items.insert(s.tgt_items.end(), items[f].begin(), items[f].end());
    s.tgt_ptr.push_back((int32_t)s.tgt_items.size());
  }
  for (size_t t = 0; t < off_items.size(); t++) {
    s.tgt_block.push_back((int32_t)off_key[t]);
    s.tgt_vertex.push_back(-1);
    s.tgt_items.insert(s.tgt_items.end(), off_items[t].begin(), off_items[t].end());
    s.tgt_ptr.push_back((int32_t)s.tgt_items.size());
  }
  std::vector<std::vector<int32_t>> ext(F);
  for (int i = 0; i < F; i++)
    for (int k = start[i]; k < i; k++) ext[k].push_back(i);
  s.ext_ptr.assign(1, 0);
  for (int k = 0; k < F; k++) {
    s.ext_rows.insert(s.ext_rows.end(), ext[k].begin(), ext[k].end());
    for (int i : ext[k]) s.ext_base.push_back(off[i] - start[i]);
    s.ext_ptr.push_back((int32_t)s.ext_rows.size());
  }
  return s;
}

}  // namespace slamgpu
