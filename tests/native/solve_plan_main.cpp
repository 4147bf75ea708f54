// Stand-alone driver of csrc/solve_plan.hpp (host code only; built by
// tests/test_solve_plan_cpu.py, with the sanitizers).  First the ChunkKey
// comparisons, one line each: "key <what> <1 if the two keys are equal>".
// Then, for every "big small need exact_rem zero_ok" line on stdin, the chunk
// lengths of that batch on one line.
#include <cstdio>

#include "solve_plan.hpp"

using namespace mfea;

int main() {
  const ChunkKey a{SolvePath::kAmg, 2, 2, 3, 1, false, false};
  auto cmp = [&](const char* what, const ChunkKey& b) { std::printf("key %s %d\n", what, a == b ? 1 : 0); };
  ChunkKey b = a;
  cmp("same", b);
  for (SolvePath p : {SolvePath::kNone, SolvePath::kCg, SolvePath::kCgParts, SolvePath::kAmgParts,
                      SolvePath::kGamgParts}) {
    b = a, b.path = p;
    cmp("path", b);
  }
  b = a, b.chunk = 4;
  cmp("chunk", b);
  b = a, b.precond = 1;
  cmp("precond", b);
  b = a, b.lanes = 2;
  cmp("lanes", b);
  b = a, b.gen = 2;
  cmp("gen", b);
  b = a, b.gen = 1000001;  // (equal to 1 once folded % 1,000,000)
  cmp("gen_folded", b);
  b = a, b.gen = (uint64_t(1) << 32) + 1;  // (equal to 1 once cut to 32 bits)
  cmp("gen_high", b);
  b = a, b.close = true;
  cmp("close", b);
  b = a, b.lazy = true;
  cmp("lazy", b);
  cmp("default", ChunkKey{});
  int big, small, need, exact_rem, zero_ok;
  while (std::scanf("%d %d %d %d %d", &big, &small, &need, &exact_rem, &zero_ok) == 5) {
    for (int n : chunk_lengths(big, small, need, exact_rem != 0, zero_ok != 0)) std::printf("%d ", n);
    std::printf("\n");
  }
  return 0;
}
