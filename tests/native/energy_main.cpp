// energy_main — csrc/energy.hpp on the host, element by element, for the tests.
//
//   energy_main <in> <out>
//
// <in>:  int64 n, then n records of 15 doubles: the coordinates of the first
//        and the second node (3 + 3), their displacements (3 + 3), EA, EI12
//        and a flag (non-zero: the element counts).
// <out>: four arrays of n doubles — w_axial, w_bending, g_axial, g_bending; an
//        element that does not count gives four zeros, as k_energy writes them.
// Built by the tests with -ffp-contract=off, the library's setting: the same
// header then yields the device's bits.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "energy.hpp"

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: energy_main <in> <out>\n");
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) {
    std::perror(argv[1]);
    return 1;
  }
  int64_t n = 0;
  if (std::fread(&n, sizeof n, 1, f) != 1 || n < 0) {
    std::fprintf(stderr, "energy_main: bad header\n");
    return 1;
  }
  std::vector<double> in(15 * (size_t)n), out(4 * (size_t)n, 0.0);
  if (std::fread(in.data(), sizeof(double), in.size(), f) != in.size()) {
    std::fprintf(stderr, "energy_main: short input\n");
    return 1;
  }
  std::fclose(f);
  for (int64_t e = 0; e < n; ++e) {
    const double* r = &in[15 * (size_t)e];
    if (r[14] == 0.0) continue;
    const mfea::ElemEnergy w = mfea::element_energy(r, r + 3, r + 6, r + 9, r[12], r[13]);
    out[e] = w.w_ax;
    out[(size_t)n + e] = w.w_b;
    out[2 * (size_t)n + e] = w.g_ax;
    out[3 * (size_t)n + e] = w.g_b;
  }
  f = std::fopen(argv[2], "wb");
  if (!f) {
    std::perror(argv[2]);
    return 1;
  }
  const bool ok = std::fwrite(out.data(), sizeof(double), out.size(), f) == out.size();
  return std::fclose(f) == 0 && ok ? 0 : 1;
}
