// solve_plan.hpp — the host-only decisions of the solve paths, stated apart
// from capi.hip: what a captured chunk graph is keyed by, and which chunk
// lengths a planned batch is queued as.  No HIP here:
// tests/native/solve_plan_main.cpp compiles it alone.  capi.hip does not
// include it yet — it still keys its graphs by the graph_chunk / graph_precond
// / graph_ell ints and computes the lengths inside drive_sized /
// drive_planned; chunk_lengths is held against those formulas by
// tests/test_solve_plan_cpu.py so that the solves can move onto it unchanged.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace mfea {

// which solve captured the chunk
enum class SolvePath : int {
  kNone = 0,
  kCg,        // one partition, CG-CG (solve_impl)
  kCgParts,   // partitioned CG-CG (solve_dist)
  kAmg,       // one partition, AMG-PCG (solve_amg)
  kAmgParts,  // partitioned, block-Jacobi AMG (solve_amg_dist)
  kGamgParts  // partitioned, one global hierarchy (solve_gamg_global)
};

// Everything a cached chunk graph depends on besides the arrays the layout
// build allocates (ensure_built destroys the graphs).  gen: a handle-global
// generation when the graph holds pointers into an AMG plan, 0 otherwise — one
// counter, monotonic, never folded, to be bumped by every plan upload and
// every layout build, so a key of an earlier plan never equals a later one's.
struct ChunkKey {
  SolvePath path = SolvePath::kNone;
  int chunk = 0;     // iterations per replay (0: the slot holds one graph per length)
  int precond = -1;  // the kernels' preconditioner argument / MFEA_PC_GAMG
  int lanes = 0;     // DOFs per node of the lane operator (0: the SELL kernels)
  uint64_t gen = 0;
  bool close = false;  // the chunk ends with the closing check
  bool lazy = false;   // p, x once per chunk (option amg_lazy_px)
  bool operator==(const ChunkKey& o) const {
    return path == o.path && chunk == o.chunk && precond == o.precond && lanes == o.lanes && gen == o.gen &&
           close == o.close && lazy == o.lazy;
  }
  bool operator!=(const ChunkKey& o) const { return !(*this == o); }
};

// The planned batch of `need` updates as chunk lengths, in queueing order:
// long chunks of `big` while a whole one fits (big > small only), then the
// remainder as ONE chunk of its own length (exact_rem) or as chunks of `small`
// — never more than small − 1 past need.  zero_ok: chunks that end with a
// closing check may be empty, need 0 is one chunk of length 0; otherwise a
// batch holds at least one update.
inline std::vector<int> chunk_lengths(int big, int small, int need, bool exact_rem, bool zero_ok) {
  need = std::max(zero_ok ? 0 : 1, need);
  if (need == 0) return {0};
  const int nbig = big > small ? need / big : 0;
  const int rem = need - nbig * big;
  std::vector<int> out((size_t)nbig, big);
  if (exact_rem && rem > 0) out.push_back(rem);
  else out.insert(out.end(), (size_t)((rem + small - 1) / small), small);
  return out;
}

}  // namespace mfea
