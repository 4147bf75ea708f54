// cube.hpp — a³ in double-double, for the host and the device.
//
// The bending stiffness divides by L_safe³ (kernels.hip bar_block) and the
// element energy by the same cube (energy.hpp): one function, so both hold the
// same bits wherever they are compiled.  The square and the cube are each
// formed with their rounding error (one fma apiece), the errors folded back
// into the result: ≈ 0.5 ulp, where NumPy's pow is ≤ 1 ulp.  These two fma are
// the only fused operations of the element arithmetic; everything else is
// built with -ffp-contract=off.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MFEA_HD __host__ __device__ __forceinline__
#else
#define MFEA_HD inline
#endif

namespace mfea {

MFEA_HD double cube(double a) {
  const double s = a * a;
  const double es = fma(a, a, -s);
  const double c = s * a;
  const double ec = fma(s, a, -c);
  return c + (ec + es * a);
}

}  // namespace mfea
