// run.hpp — the device side of mfea_run (capi.hip): one step's record rows
// (displacement in original node order, stress, activity) gathered into a
// staging slab on the handle's stream, for a second stream to copy out while
// the next step computes.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mfea {

// One staging slab: U row (3·N f64) | stress row (E f64) | activity row (E u8).
// Offsets in bytes; every f64 row starts on a multiple of 8.
struct RecordSlab {
  int64_t off_u = 0, off_s = 0, off_a = 0, bytes = 0;
};
inline RecordSlab record_slab(int64_t n_nodes, int64_t n_elems) {
  RecordSlab L;
  L.off_u = 0;
  L.off_s = 24 * n_nodes;
  L.off_a = L.off_s + 8 * n_elems;
  L.bytes = L.off_a + n_elems;
  return L;
}

// u_row[3g + a] = x[3·iperm[g] + a] for every original node g (iperm[g] in
// [0, N): the permuted row of node g); s_row = stress, a_row = active (both in
// element order already on one partition).  A row pointer may be NULL (not
// kept).  One launch; nothing is launched for N == 0 and E == 0.
void launch_record_step(hipStream_t s, int64_t N, const int32_t* iperm, const double* x, double* u_row,
                        int64_t E, const double* stress, double* s_row, const uint8_t* active,
                        uint8_t* a_row);

// The rows of an event (mfea_run_events): as launch_record_step, with
// u_row[3g + a] = *lam · x[3·iperm[g] + a] (lam: device memory).
void launch_record_event(hipStream_t s, int64_t N, const int32_t* iperm, const double* x, const double* lam,
                         double* u_row, int64_t E, const double* stress, double* s_row,
                         const uint8_t* active, uint8_t* a_row);

}  // namespace mfea
