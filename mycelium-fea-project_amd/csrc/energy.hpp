// energy.hpp — strain energy of one element, for the host and the device.
//
// The element's block is S = k_ax nnᵀ + k_b (I − nnᵀ) (kernels.hip bar_block),
// so with δ = u_b − u_a its energy ½ δᵀSδ splits into an axial part
// ½ k_ax d² (d = n·δ) and a transverse part ½ k_b |δ − d n|².  Per unit section
// the two are g_ax and g_b; w = section · g, one product each, so the relation
// is exact in bits and g is the energy's derivative with respect to EA_e / EI12_e
// at fixed U (include/mfea.h mfea_get_energy: why that is the gradient of the
// equilibrium energy too).
//
// Every operation below is one IEEE f64 operation in the order written — the
// tree builds with -ffp-contract=off — except inside cube (cube.hpp).  The
// length is bar_block's expression, so L_safe and n have K's bits.  The
// transverse part is formed as a vector, not as |δ|² − d²: under tension the
// two terms of that difference agree to many digits.
// L == 0: n = 0, d = 0, t = δ and w_b = ½ k_b |δ|², what K holds for the
// element; the result is finite wherever K is.
#pragma once
#include "cube.hpp"

namespace mfea {

struct ElemEnergy {
  double w_ax, w_b;  // EA·g_ax, EI12·g_b
  double g_ax, g_b;  // energy per unit EA, per unit EI12
};

// pa, pb: the coordinates of the element's first and second node (n1, n2 of
// elements.csv); ua, ub: their displacements
MFEA_HD ElemEnergy element_energy(const double pa[3], const double pb[3], const double ua[3], const double ub[3],
                                  double EA, double EI12) {
  const double vx = pb[0] - pa[0], vy = pb[1] - pa[1], vz = pb[2] - pa[2];
  const double L = sqrt(vx * vx + vy * vy + vz * vz);
  const double Ls = L < 1e-12 ? 1e-12 : L;
  const double n0 = vx / Ls, n1 = vy / Ls, n2 = vz / Ls;
  const double d0 = ub[0] - ua[0], d1 = ub[1] - ua[1], d2 = ub[2] - ua[2];
  const double d = (n0 * d0 + n1 * d1) + n2 * d2;
  const double t0 = d0 - d * n0, t1 = d1 - d * n1, t2 = d2 - d * n2;
  const double q = (t0 * t0 + t1 * t1) + t2 * t2;
  ElemEnergy r;
  r.g_ax = ((0.5 * d) * d) / Ls;
  r.g_b = (0.5 * q) / cube(Ls);
  r.w_ax = EA * r.g_ax;
  r.w_b = EI12 * r.g_b;
  return r;
}

}  // namespace mfea
