// events.hip — the post of an event-driven failure run (mfea_event /
// mfea_run_events, capi.hip).  Between failures the problem is
// linear in the grip displacement, so one solve at a reference load gives the
// load factor at which the most strained element reaches the failure strain:
//
//   k_event_scan   F₁ = Σ_top (K·U₁)_y  and  smax = max |ε_e| over the active
//                  elements, one launch over two row sets;
//   k_event_apply  lam = max_strain / smax, the failing group, the stress row
//                  at the failure load, #active — reads smax from device
//                  memory, so no host round trip lies between the two.
//
// With a per-element strength (mfea_set_element_props, max_strain) the pair
// runs in its second form: the scan reduces lam = min_e max_strain_e / |ε_e|
// (identity +inf) where it reduced smax, and the apply fails every element
// with lam_e <= lam / (1 − tie_rtol).  Both forms are template instantiations;
// the uniform one is the code it was.
//
// Every expression below is one IEEE f64 operation (the build disables
// contraction), so NumPy reproduces the results bit for bit.
#include "kernels.hpp"
#include "device_util.hpp"

#include <math.h>

namespace mfea {

namespace {

// ε of element e from the solution, k_stress's chain (kernels.hip): n = v/L,
// the dot product as BLAS ddot forms it, ε = (n·Δu)/L.  Every load is issued
// whatever the element's state; the caller masks the result.
__device__ __forceinline__ double element_strain(const int32_t* __restrict__ e2n, const double* __restrict__ xyz,
                                                 const double* __restrict__ u, int64_t e, bool* valid) {
  int32_t a = e2n[2 * e], b = e2n[2 * e + 1];
  *valid = a >= 0;
  a = a < 0 ? 0 : a;
  b = b < 0 ? 0 : b;
  const double ax = xyz[3 * a], ay = xyz[3 * a + 1], az = xyz[3 * a + 2];
  const double bx = xyz[3 * b], by = xyz[3 * b + 1], bz = xyz[3 * b + 2];
  const double ua0 = u[3 * a], ua1 = u[3 * a + 1], ua2 = u[3 * a + 2];
  const double ub0 = u[3 * b], ub1 = u[3 * b + 1], ub2 = u[3 * b + 2];
  const double vx = bx - ax, vy = by - ay, vz = bz - az;
  const double L = sqrt(fma(vz, vz, fma(vy, vy, vx * vx)));
  const double n0 = vx / L, n1 = vy / L, n2 = vz / L;
  const double du0 = ub0 - ua0, du1 = ub1 - ua1, du2 = ub2 - ua2;
  const double dot = fma(n2, du2, fma(n1, du1, n0 * du0));
  return dot / L;
}

// max over the block, result on thread 0 (a max is order-free: any tree gives
// the same bits); MIN: the min instead (identity +inf), order-free likewise
template <bool MIN = false>
__device__ __forceinline__ double block_max(double v, double* lds) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = MIN ? fmin(v, __shfl_xor(v, o)) : fmax(v, __shfl_xor(v, o));
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) lds[wid] = v;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < kBlock / 64; ++w) v = MIN ? fmin(v, lds[w]) : fmax(v, lds[w]);
  return v;
}

// ---------------------------------------------------------------------------
// One launch, two row sets.  Blocks [0, grid_r): the top grip rows, k_reaction's
// body and its reduction over grid_r blocks — F₁ has the bits mfea_post gives.
// Blocks [grid_r, grid_r + grid_e): the elements — ε_e (kept in `eps` when
// given), the block's max |ε| over active elements (NaN skipped) and its
// number of active elements; the block that finishes the count's reduction
// (every element block has published by then) takes the max of the block maxima.
// PS (q.strength): lam_e = max_strain_e / |ε_e| of the same elements and the
// min in place of the max, through the same publish.
// GM = GripVec (q.vec): the row blocks run k_reaction<GripVec>'s body — the
// reaction vector into q.sums, F₁ along q.w into force_out, the same bits.
// GM = GripField (q.field): k_reaction<GripField>'s body — F₁ = Σ w_r of the top
// rows into force_out through the scalar publish, the same bits.
// ---------------------------------------------------------------------------
template <bool PS, class GM>
__global__ __launch_bounds__(kBlock) void k_event_scan(EventScan q) {
  __shared__ double mx[kBlock / 64];
  if (blockIdx.x < q.grid_r) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if constexpr (std::is_same<GM, GripVec>::value) {
      double f3[3] = {0.0, 0.0, 0.0};
      if (t < q.nrows)
        reaction_row3(q.row0 + t, q.N, q.slice_ptr, q.row_len, q.s_col, q.val, q.diag, q.G, q.u, f3);
      reaction3_publish(f3, q.partials_r, q.ticket_r, q.sums, q.w, q.force_out, q.grid_r, blockIdx.x);
      return;
    }
    if constexpr (std::is_same<GM, GripField>::value) {
      double w[1] = {0.0};
      if (t < q.nrows) {
        double f3[3];
        reaction_row3(q.row0 + t, q.N, q.slice_ptr, q.row_len, q.s_col, q.val, q.diag, q.G, q.u, f3);
        w[0] = grip_work_row(q.field + 3 * t, f3);
      }
      block_publish_as<1>(w, q.partials_r, q.ticket_r, q.force_out, q.grid_r, blockIdx.x);
      return;
    }
    double f[1] = {0.0};
    if (t < q.nrows) {
      const int64_t N = q.N, G = q.G;
      const int64_t row = q.row0 + t;
      const int64_t base = (int64_t)q.slice_ptr[row >> 6] * 64 + (row & 63);
      const int len = q.row_len[row];
      double fy = q.diag[N + row] * q.u[3 * row] + q.diag[3 * N + row] * q.u[3 * row + 1] +
                  q.diag[4 * N + row] * q.u[3 * row + 2];
      // (slots in batches of four, terms in slot order: see k_reaction)
      constexpr int U = 4;
      for (int k0 = 0; k0 < len; k0 += U) {
        int64_t idx[U], c[U];
#pragma unroll
        for (int j = 0; j < U; ++j) {
          idx[j] = base + (int64_t)(k0 + j < len ? k0 + j : k0) * 64;
          c[j] = q.s_col[idx[j]];
        }
        double tm[U];
#pragma unroll
        for (int j = 0; j < U; ++j)
          tm[j] = q.val[G + idx[j]] * q.u[3 * c[j]] + q.val[3 * G + idx[j]] * q.u[3 * c[j] + 1] +
                  q.val[4 * G + idx[j]] * q.u[3 * c[j] + 2];
#pragma unroll
        for (int j = 0; j < U; ++j)
          if (k0 + j < len) fy += tm[j];
      }
      f[0] = fy;
    }
    block_publish_as<1>(f, q.partials_r, q.ticket_r, q.force_out, q.grid_r, blockIdx.x);
    return;
  }
  const unsigned be = blockIdx.x - q.grid_r;
  const int64_t e = (int64_t)be * kBlock + threadIdx.x;
  double cnt[1] = {0.0};
  double m = PS ? (double)INFINITY : 0.0;
  if (q.E > 0) {
    const bool in = e < q.E;
    const int64_t ec = in ? e : q.E - 1;
    const uint8_t act = q.active[ec];
    bool valid;
    const double strain = element_strain(q.e2n, q.xyz, q.u, ec, &valid);
    if (q.eps && in) q.eps[e] = strain;
    const double as = fabs(strain);
    // (a NaN strain — a zero-length element — compares false: skipped)
    if constexpr (PS) {
      const double ms = q.strength[ec];
      if (in && act && valid && as > 0.0) m = ms / as;
    } else {
      if (in && act && valid && as > 0.0) m = as;
    }
    cnt[0] = (in && act) ? 1.0 : 0.0;
  }
  m = block_max<PS>(m, mx);
  if (threadIdx.x == 0) store_sc1(&q.pmax[be], m);
  // (thread 0 drains its stores — the block maximum among them — before its
  // ticket in block_publish_as)
  if (!block_publish_as<1>(cnt, q.partials_e, q.ticket_e, q.cnt_out, q.grid_e, be)) return;
  double r = PS ? (double)INFINITY : 0.0;
  for (unsigned k = threadIdx.x; k < q.grid_e; k += kBlock)
    r = PS ? fmin(r, load_sc1(&q.pmax[k])) : fmax(r, load_sc1(&q.pmax[k]));
  r = block_max<PS>(r, mx);
  if (threadIdx.x == 0) *q.smax_out = r;
}

// ---------------------------------------------------------------------------
// The event's decision and records.  lam = max_strain / smax (+inf on an
// unloaded network).  When lam <= lam_max and the network is loaded, every
// active element with |ε| >= smax·(1 − tie_rtol) fails: its activity is
// cleared, event_of[e] = k, and it joins the failed-element list as in
// k_stress.  Otherwise the event is terminal and no activity is touched.
// stress = (E·ε)·lam for elements active at event start (terminal: the factor
// is lam_max when finite, else 1), 0 otherwise.  Reduces #active (after).
// PS (q.strength): *q.smax holds the scan's lam = min lam_e (+inf: no loaded
// element of finite strength — terminal); the group is every active, valid
// element with |ε| > 0 and lam_e = max_strain_e / |ε_e| <= lam / (1 − tie_rtol).
// PM (q.Ee): E_e in the stress row.
// ---------------------------------------------------------------------------
template <bool PS, bool PM>
__global__ __launch_bounds__(kBlock) void k_event_apply(EventApply q) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const double smax = *q.smax;
  const double lam = PS ? smax : q.max_strain / smax;
  const bool breaks = PS ? (lam < (double)INFINITY && lam <= q.lam_max) : (smax > 0.0 && lam <= q.lam_max);
  const double thr = PS ? lam / (1.0 - q.tie_rtol) : smax * (1.0 - q.tie_rtol);
  const double factor = breaks ? lam : (isfinite(q.lam_max) ? q.lam_max : 1.0);
  if (blockIdx.x == 0 && threadIdx.x == 0) *q.lam_out = lam;
  double cnt[1] = {0.0};
  if (q.E > 0) {
    const bool in = e < q.E;
    const int64_t ec = in ? e : q.E - 1;
    const uint8_t act0 = q.active[ec];
    bool valid;
    double strain;
    if (q.eps) {
      strain = q.eps[ec];
      valid = q.e2n[2 * ec] >= 0;
    } else {
      strain = element_strain(q.e2n, q.xyz, q.u, ec, &valid);
    }
    double Em = q.Emod, ms = 0.0;
    if constexpr (PM) Em = q.Ee[ec];
    if constexpr (PS) ms = q.strength[ec];
    if (in) {
      const bool live = act0 && valid;
      const double as = fabs(strain);
      const bool fails = PS ? (live && breaks && as > 0.0 && ms / as <= thr) : (live && breaks && as >= thr);
      q.stress[e] = live ? (Em * strain) * factor : 0.0;
      if (fails) {
        q.active[e] = 0;
        q.event_of[e] = q.k;
        q.fail_list[atomicAdd(q.fail_cnt, 1u)] = (int32_t)e;
      }
      cnt[0] = (act0 && !fails) ? 1.0 : 0.0;
    }
  }
  block_publish<1>(cnt, q.partials, q.ticket, q.cnt_out);
}

// Undo an event's failures (capi.hip spec_undo), as k_unfail does for a post:
// the listed elements are active again, belong to no event, the list is empty.
__global__ __launch_bounds__(kBlock) void k_event_unfail(const int32_t* __restrict__ fail_list, unsigned* cnt,
                                                         uint8_t* __restrict__ active,
                                                         int32_t* __restrict__ event_of) {
  const unsigned c = *cnt;
  for (unsigned k = threadIdx.x; k < c; k += kBlock) {
    active[fail_list[k]] = 1;
    event_of[fail_list[k]] = -1;
  }
  __syncthreads();
  if (threadIdx.x == 0) *cnt = 0u;
}

}  // namespace

void launch_event_scan(hipStream_t s, EventScan q) {
  if (q.field) q.vec = false;  // (a grip field: one sum, the scalar partial area)
  q.grid_r = (unsigned)grid_rows(q.nrows > 0 ? q.nrows : 1);
  q.grid_e = (unsigned)grid_rows(q.E > 0 ? q.E : 1);
  // the two row sets reduce side by side: disjoint partials
  q.partials_r = q.partials;
  q.partials_e = q.partials_r + (q.vec ? 3 : 1) * (q.grid_r + kShards);  // (three sums: three times the room)
  q.pmax = q.partials_e + (q.grid_e + kShards);
  const dim3 g(q.grid_r + q.grid_e);
  // (only the form's type is read: the kernel takes w and the field from q)
  const GripVec vec{};
  with_grip(BcForm{q.vec ? &vec : nullptr, q.field, nullptr}, [&](auto gm) {
    using GM = decltype(gm);
    if (q.strength) hipLaunchKernelGGL((k_event_scan<true, GM>), g, dim3(kBlock), 0, s, q);
    else hipLaunchKernelGGL((k_event_scan<false, GM>), g, dim3(kBlock), 0, s, q);
  });
}

int64_t event_scan_partials(int64_t n_top, int64_t n_elems, bool vec) {
  return (vec ? 3 : 1) * (grid_rows(n_top > 0 ? n_top : 1) + kShards) + 2 * grid_rows(n_elems > 0 ? n_elems : 1) +
         kShards;
}

void launch_event_apply(hipStream_t s, const EventApply& q) {
  const dim3 g((unsigned)grid_rows(q.E > 0 ? q.E : 1));
  auto k = q.strength ? (q.Ee ? k_event_apply<true, true> : k_event_apply<true, false>)
                      : (q.Ee ? k_event_apply<false, true> : k_event_apply<false, false>);
  hipLaunchKernelGGL(k, g, dim3(kBlock), 0, s, q);
}

void launch_event_unfail(hipStream_t s, const int32_t* fail_list, unsigned* cnt, uint8_t* active,
                         int32_t* event_of) {
  hipLaunchKernelGGL(k_event_unfail, dim3(1), dim3(kBlock), 0, s, fail_list, cnt, active, event_of);
}

}  // namespace mfea
