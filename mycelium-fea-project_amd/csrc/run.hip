// run.hip — the record gather of mfea_run (run.hpp).
#include "run.hpp"

#include <algorithm>

#include "kernels.hpp"

namespace mfea {

namespace {

// One thread per original node g: a 24-byte gather from the permuted solution
// (4 + 24 bytes read), three consecutive doubles written — a wave writes one
// contiguous 1536-byte run.  Then one thread per element: the stress and the
// activity as they stand (9 bytes read, 9 written).  52·N + 18·E bytes in all.
__global__ __launch_bounds__(kBlock) void k_record_step(int64_t N, const int32_t* __restrict__ iperm,
                                                        const double* __restrict__ x,
                                                        double* __restrict__ u_row, int64_t E,
                                                        const double* __restrict__ stress,
                                                        double* __restrict__ s_row,
                                                        const uint8_t* __restrict__ active,
                                                        uint8_t* __restrict__ a_row) {
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (u_row) {
    for (int64_t g = t0; g < N; g += stride) {
      const int64_t i = iperm[g];
      const double a = x[3 * i], b = x[3 * i + 1], c = x[3 * i + 2];
      u_row[3 * g] = a;
      u_row[3 * g + 1] = b;
      u_row[3 * g + 2] = c;
    }
  }
  if (s_row)
    for (int64_t e = t0; e < E; e += stride) s_row[e] = stress[e];
  if (a_row)
    for (int64_t e = t0; e < E; e += stride) a_row[e] = active[e];
}

// The same rows for an event (mfea_run_events): the displacement at the
// failure load, u_row = lam · x with the event's load factor read from device
// memory (k_event_apply's lam_out) — one multiply per entry.
__global__ __launch_bounds__(kBlock) void k_record_event(int64_t N, const int32_t* __restrict__ iperm,
                                                         const double* __restrict__ x,
                                                         const double* __restrict__ lam_p,
                                                         double* __restrict__ u_row, int64_t E,
                                                         const double* __restrict__ stress,
                                                         double* __restrict__ s_row,
                                                         const uint8_t* __restrict__ active,
                                                         uint8_t* __restrict__ a_row) {
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (u_row) {
    const double lam = *lam_p;
    for (int64_t g = t0; g < N; g += stride) {
      const int64_t i = iperm[g];
      const double a = x[3 * i], b = x[3 * i + 1], c = x[3 * i + 2];
      u_row[3 * g] = lam * a;
      u_row[3 * g + 1] = lam * b;
      u_row[3 * g + 2] = lam * c;
    }
  }
  if (s_row)
    for (int64_t e = t0; e < E; e += stride) s_row[e] = stress[e];
  if (a_row)
    for (int64_t e = t0; e < E; e += stride) a_row[e] = active[e];
}

}  // namespace

void launch_record_event(hipStream_t s, int64_t N, const int32_t* iperm, const double* x, const double* lam,
                         double* u_row, int64_t E, const double* stress, double* s_row,
                         const uint8_t* active, uint8_t* a_row) {
  if (N <= 0) u_row = nullptr;
  if (E <= 0) s_row = nullptr, a_row = nullptr;
  if (!u_row && !s_row && !a_row) return;
  const int64_t n = std::max<int64_t>(u_row ? N : 0, (s_row || a_row) ? E : 0);
  hipLaunchKernelGGL(k_record_event, dim3((unsigned)grid_elementwise(n)), dim3(kBlock), 0, s, N, iperm, x,
                     lam, u_row, E, stress, s_row, active, a_row);
}

void launch_record_step(hipStream_t s, int64_t N, const int32_t* iperm, const double* x, double* u_row,
                        int64_t E, const double* stress, double* s_row, const uint8_t* active,
                        uint8_t* a_row) {
  if (N <= 0) u_row = nullptr;
  if (E <= 0) s_row = nullptr, a_row = nullptr;
  if (!u_row && !s_row && !a_row) return;
  const int64_t n = std::max<int64_t>(u_row ? N : 0, (s_row || a_row) ? E : 0);
  hipLaunchKernelGGL(k_record_step, dim3((unsigned)grid_elementwise(n)), dim3(kBlock), 0, s, N, iperm, x,
                     u_row, E, stress, s_row, active, a_row);
}

}  // namespace mfea
