// device_util.hpp — device helpers shared by the mfea kernels (wave64 reductions,
// fence-free sharded last-block finalize, symmetric 3×3 block algebra).
#pragma once
#include <type_traits>

#include "kernels.hpp"

namespace mfea {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// DPP move of a double (two 32-bit halves), all lanes active
template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double readlane_d(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}
// Wave total in every lane, in a fixed order (identical in every wave):
// quad sums by quad_perm, 8- and 16-lane sums by row_half_mirror / row_mirror
// (each step pairs two equal-order partial sums, so all lanes of a row agree
// bitwise), then the four row sums read out as scalars.  VALU only: no LDS
// round trips (a __shfl_xor butterfly is 12 ds_bpermute_b32 per double).
__device__ __forceinline__ double wave_allsum(double v) {
  v += dpp_d<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_d<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_d<0x141>(v);  // row_half_mirror
  v += dpp_d<0x140>(v);  // row_mirror
  return (readlane_d(v, 0) + readlane_d(v, 16)) + (readlane_d(v, 32) + readlane_d(v, 48));
}

// Ticket layout: one ticket set = kTicketStride unsigned; shard s counter at
// s·16 (64 B apart, separate lines), the top counter at kShards·16.
constexpr int kShards = 8;
static_assert((kShards + 1) * 16 <= kTicketStride, "ticket set too small");

// Sum over the block of NV values, result on thread 0 (others: garbage).
template <int NV, int BS>
__device__ __forceinline__ void block_sum(double (&v)[NV], double* lds) {
  constexpr int NW = BS / 64;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < NV; ++c) v[c] = wave_sum(v[c]);
  if (NW > 1) {
    __syncthreads();
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < NV; ++c) lds[wid * NV + c] = v[c];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
      for (int c = 0; c < NV; ++c) {
        double s = lds[c];
        for (int w = 1; w < NW; ++w) s += lds[w * NV + c];
        v[c] = s;
      }
    }
  }
}

__device__ __forceinline__ void store_sc1(double* p, double v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double load_sc1(const double* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------
// Deterministic grid reduction finished inside the launch (no second kernel):
// every block publishes its partial sums; the last arriver of each of
// kShards shards (blocks ≡ s mod kShards) sums its shard's partials in block
// order and publishes a shard sum; the last shard finisher sums the shard sums
// in shard order and writes `out`.  Bitwise reproducible for a fixed grid.
//
// Two levels because same-address agent atomics serialize at ≈12 ns each
// (MI355X_MICROARCH.md, row "fanin"): one counter for 1,300 blocks costs
// ≈16 µs; eight shards of ≤165 plus a top counter of 8 cost ≈2 µs.
//
// Hand-off without fences (MI355X_MICROARCH.md "Valid forms", table row 1):
// payload stored write-through (sc1, agent-scope atomic stores), the storing
// lane drains it (s_waitcnt vmcnt(0)) before its agent-scope ticket add, the
// last arriver reads every payload word with sc1 loads.  No ≈1.7 µs
// release/acquire fence on the per-iteration path.
// partials must hold NV·(gridDim + kShards) doubles.
// ---------------------------------------------------------------------------
// block_publish_as: the same over blocks b = 0..G-1 of a launch that holds
// other blocks too (k_event_scan's two row sets: each set reduces as its own
// kernel would, with its own partials and ticket set).
template <int NV, int BS = kBlock>
__device__ __forceinline__ bool block_publish_as(double (&v)[NV], double* partials, unsigned* ticket,
                                                 double* out, const unsigned G, const unsigned b) {
  constexpr int NW = BS / 64;
  __shared__ double lds[NW * NV];
  __shared__ int flag;
  const unsigned S = G < (unsigned)kShards ? G : (unsigned)kShards;
  const unsigned shard = b % S;
  const unsigned nshard = (G - shard + S - 1) / S;
  double* spart = partials + (size_t)NV * G;  // shard sums, [c][S]

  block_sum<NV, BS>(v, lds);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < NV; ++c) store_sc1(&partials[(size_t)c * G + b], v[c]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned t =
        __hip_atomic_fetch_add(&ticket[shard * 16], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    flag = (t == nshard - 1);
  }
  __syncthreads();
  if (!flag) return false;

  // ---- last block of this shard: sum its blocks' partials in block order
  constexpr int U = BS >= 256 ? 4 : 8;
  double s[NV];
#pragma unroll
  for (int c = 0; c < NV; ++c) s[c] = 0.0;
  for (unsigned k0 = threadIdx.x; k0 < nshard; k0 += BS * U) {
    double t[U][NV];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const unsigned k = k0 + u * BS;
      const unsigned blk = shard + k * S;
#pragma unroll
      for (int c = 0; c < NV; ++c) t[u][c] = k < nshard ? load_sc1(&partials[(size_t)c * G + blk]) : 0.0;
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int c = 0; c < NV; ++c) s[c] += t[u][c];
  }
  block_sum<NV, BS>(s, lds);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < NV; ++c) store_sc1(&spart[c * S + shard], s[c]);
    __hip_atomic_store(&ticket[shard * 16], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned t = __hip_atomic_fetch_add(&ticket[kShards * 16], 1u, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT);
    flag = (t == S - 1);
  }
  __syncthreads();
  if (!flag) return false;

  // ---- last shard finisher: shard sums in shard order
  if (threadIdx.x == 0) {
    double r[NV];
#pragma unroll
    for (int c = 0; c < NV; ++c) r[c] = 0.0;
    for (unsigned q = 0; q < S; ++q)
#pragma unroll
      for (int c = 0; c < NV; ++c) r[c] += load_sc1(&spart[c * S + q]);
#pragma unroll
    for (int c = 0; c < NV; ++c) out[c] = r[c];
    __hip_atomic_store(&ticket[kShards * 16], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  return true;
}

template <int NV, int BS = kBlock>
__device__ __forceinline__ bool block_publish(double (&v)[NV], double* partials,
                                              unsigned* ticket, double* out) {
  return block_publish_as<NV, BS>(v, partials, ticket, out, gridDim.x, blockIdx.x);
}

// (K·U)[3·row + c], c = 0..2, of Pattern row `row` on the unregularised K
// (k_reaction<GripVec>, kernels.hip; k_event_scan<·, GripVec>, events.hip):
// every block row accumulated as k_reaction accumulates its y row — the
// diagonal block's three products, then the slots in batches of four, each
// batch's columns and values issued before its gathers, terms in slot order.
__device__ __forceinline__ void reaction_row3(int64_t row, int64_t N, const int32_t* __restrict__ slice_ptr,
                                              const int32_t* __restrict__ row_len,
                                              const int32_t* __restrict__ s_col, const double* __restrict__ val,
                                              const double* __restrict__ diag, int64_t G,
                                              const double* __restrict__ u, double f[3]) {
  const int64_t base = (int64_t)slice_ptr[row >> 6] * 64 + (row & 63);
  const int len = row_len[row];
  {
    double d[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) d[c] = diag[(int64_t)c * N + row];
    const double u0 = u[3 * row], u1 = u[3 * row + 1], u2 = u[3 * row + 2];
    f[0] = d[0] * u0 + d[1] * u1 + d[2] * u2;
    f[1] = d[1] * u0 + d[3] * u1 + d[4] * u2;
    f[2] = d[2] * u0 + d[4] * u1 + d[5] * u2;
  }
  constexpr int U = 4;
  for (int k0 = 0; k0 < len; k0 += U) {
    int64_t idx[U], c[U];
#pragma unroll
    for (int q = 0; q < U; ++q) {
      idx[q] = base + (int64_t)(k0 + q < len ? k0 + q : k0) * 64;
      c[q] = s_col[idx[q]];
    }
    double t[U][3];
#pragma unroll
    for (int q = 0; q < U; ++q) {
      double v[6];
#pragma unroll
      for (int a = 0; a < 6; ++a) v[a] = val[(int64_t)a * G + idx[q]];
      const double u0 = u[3 * c[q]], u1 = u[3 * c[q] + 1], u2 = u[3 * c[q] + 2];
      t[q][0] = v[0] * u0 + v[1] * u1 + v[2] * u2;
      t[q][1] = v[1] * u0 + v[3] * u1 + v[4] * u2;
      t[q][2] = v[2] * u0 + v[4] * u1 + v[5] * u2;
    }
#pragma unroll
    for (int q = 0; q < U; ++q)
      if (k0 + q < len) {
#pragma unroll
        for (int a = 0; a < 3; ++a) f[a] += t[q][a];
      }
  }
}

// ... reduced over the G blocks into sums[0..2]; the block that ends the
// reduction forms the work-conjugate force along w into force_out (or NULL):
//   F = (w[0]·sums[0] + w[1]·sums[1]) + w[2]·sums[2]
__device__ __forceinline__ void reaction3_publish(double (&f)[3], double* partials, unsigned* ticket, double* sums,
                                                  const double w[3], double* force_out, unsigned G, unsigned b) {
  if (!block_publish_as<3>(f, partials, ticket, sums, G, b)) return;
  if (threadIdx.x == 0 && force_out) *force_out = (w[0] * sums[0] + w[1] * sums[1]) + w[2] * sums[2];
}

__device__ __forceinline__ void sym_apply(const double B[6], const double v[3], double o[3]) {
  o[0] = fma(B[0], v[0], fma(B[1], v[1], B[2] * v[2]));
  o[1] = fma(B[1], v[0], fma(B[3], v[1], B[4] * v[2]));
  o[2] = fma(B[2], v[0], fma(B[4], v[1], B[5] * v[2]));
}

__device__ __forceinline__ void sym_inverse(const double A[6], double B[6]) {
  // adjugate / determinant of a symmetric 3×3 (SPD here)
  const double c00 = A[3] * A[5] - A[4] * A[4];
  const double c01 = A[2] * A[4] - A[1] * A[5];
  const double c02 = A[1] * A[4] - A[2] * A[3];
  const double c11 = A[0] * A[5] - A[2] * A[2];
  const double c12 = A[1] * A[2] - A[0] * A[4];
  const double c22 = A[0] * A[3] - A[1] * A[1];
  const double det = A[0] * c00 + A[1] * c01 + A[2] * c02;
  const double id = 1.0 / det;
  B[0] = c00 * id; B[1] = c01 * id; B[2] = c02 * id;
  B[3] = c11 * id; B[4] = c12 * id; B[5] = c22 * id;
}

// Grip motion (kernels.hpp GripVec): the two prescribed displacements of a
// launch, p[c] = fl(amplitude · direction[c]) — one product per component
struct GripP {
  double top[3], bot[3];
};
__device__ __forceinline__ GripP grip_disp(const GripVec& g, double dy_top, double dy_bot) {
  GripP p;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    p.top[c] = dy_top * g.top[c];
    p.bot[c] = dy_bot * g.bot[c];
  }
  return p;
}
// the prescribed displacement of a row of class `code` (1 top, 2 bottom, 3 a
// ghost free row: 0) — selects on registers, no indexed access
__device__ __forceinline__ void grip_of(const GripP& p, uint8_t code, double x[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) x[c] = code == 3 ? 0.0 : (code == 2 ? p.bot[c] : p.top[c]);
}
// Grip field (kernels.hpp GripField): the prescribed displacement of known row
// `row` of class `code` (3: 0) from its vector d = g.d + 3·(row − nf) —
// p[c] = fl(amp · d[c]), amp by the class, one product per component
__device__ __forceinline__ double grip_amp(uint8_t code, double dy_top, double dy_bot) {
  return code == 2 ? dy_bot : dy_top;
}
__device__ __forceinline__ void grip_of(const double d[3], uint8_t code, double dy_top, double dy_bot, double x[3]) {
  const double amp = grip_amp(code, dy_top, dy_bot);
#pragma unroll
  for (int c = 0; c < 3; ++c) x[c] = code == 3 ? 0.0 : amp * d[c];
}
__device__ __forceinline__ void grip_of(const GripField& g, int64_t row, int64_t nf, uint8_t code, double dy_top,
                                        double dy_bot, double x[3]) {
  const double d[3] = {g.d[3 * (row - nf)], g.d[3 * (row - nf) + 1], g.d[3 * (row - nf) + 2]};
  grip_of(d, code, dy_top, dy_bot, x);
}
// the generalised force of one row: w = (d·f), f64 products and sums in this
// order, nothing fused (k_reaction<GripField>, k_event_scan<·, GripField>)
__device__ __forceinline__ double grip_work_row(const double* __restrict__ d, const double f[3]) {
  return (d[0] * f[0] + d[1] * f[1]) + d[2] * f[2];
}

// k += V p with V a known neighbour's symmetric block (v0..v5): the RHS term of
// every GripVec kernel, each row's three terms in component order
__device__ __forceinline__ void grip_mac(const double v[6], const double p[3], double k[3]) {
  k[0] = fma(v[2], p[2], fma(v[1], p[1], fma(v[0], p[0], k[0])));
  k[1] = fma(v[4], p[2], fma(v[3], p[1], fma(v[1], p[0], k[1])));
  k[2] = fma(v[5], p[2], fma(v[4], p[1], fma(v[2], p[0], k[2])));
}

// Nodal loads (kernels.hpp NodeLoad): a free row's three stored doubles and its
// mask byte, fetched where the row's first loads are issued (the slot pointer
// and the row length), not behind the slot loop — nothing else depends on them
// before the loop ends.  LoadNone: nothing is loaded and b = 0 − k.
template <class LD>
struct LoadRow {};
template <>
struct LoadRow<NodeLoad> {
  double f[3];
  uint8_t fl;
};
__device__ __forceinline__ LoadRow<LoadNone> load_fetch(const LoadNone&, int64_t) { return {}; }
__device__ __forceinline__ LoadRow<NodeLoad> load_fetch(const NodeLoad& ld, int64_t row) {
  LoadRow<NodeLoad> r;
#pragma unroll
  for (int c = 0; c < 3; ++c) r.f[c] = ld.f[3 * row + c];
  r.fl = ld.fl[row];
  return r;
}
// q of the row: one product per component (amp 1 for a dead load), 0 on a
// floating row; + 0 turns a product −0 into 0
__device__ __forceinline__ void load_q(const NodeLoad& ld, const LoadRow<NodeLoad>& lr, double dy_top, double q[3]) {
  const double amp = ld.prop ? dy_top : 1.0;
#pragma unroll
  for (int c = 0; c < 3; ++c) q[c] = lr.fl ? 0.0 : amp * lr.f[c] + 0.0;
}
// b = q − k (LoadNone: 0 − k), one subtraction per component
__device__ __forceinline__ void load_rhs(const LoadNone&, const LoadRow<LoadNone>&, double, const double k[3],
                                         double b[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) b[c] = 0.0 - k[c];
}
__device__ __forceinline__ void load_rhs(const NodeLoad& ld, const LoadRow<NodeLoad>& lr, double dy_top,
                                         const double k[3], double b[3]) {
  double q[3];
  load_q(ld, lr, dy_top, q);
#pragma unroll
  for (int c = 0; c < 3; ++c) b[c] = q[c] - k[c];
}

// b = 0 − K_fk x_k of free row `row` for the GAMG solves (k_amg_rhs, cg.hip;
// k_amg_start, amg.hip).  A row's slots in batches of four: columns, then
// their codes, then the known couplings; b's terms in slot order.
// GM = GripVec (p: the two prescribed displacements): the whole block, grip_mac.
// GM = GripField (fd: the field's rows): the same with p per neighbour — the
// vectors of a batch's four neighbours loaded together after the codes, every
// load unconditional on an index clamped into the known rows, the class applied
// after (a guarded load would serialise the batch).
// LD = NodeLoad (ld): b = q − k, the row's load fetched with its first loads.
template <class GM = GripY, class LD = LoadNone>
__device__ __forceinline__ void amg_rhs_row(const SellOp& op, const uint8_t* __restrict__ code, double dy_top,
                                            double dy_bot, int64_t row, double b[3], const GripP* p = nullptr,
                                            const double* __restrict__ fd = nullptr, const LD& ld = LD{}) {
  const int64_t base = (int64_t)op.slice_ptr[row >> 6] * 64 + (row & 63);
  const int len = op.row_len[row];
  const LoadRow<LD> lr = load_fetch(ld, row);
  const int64_t G = op.G;
  double kx = 0.0, ky = 0.0, kz = 0.0;
  if constexpr (std::is_same<GM, GripField>::value) {
    double k3[3] = {0.0, 0.0, 0.0};
    constexpr int U = 4;
    for (int k0 = 0; k0 < len; k0 += U) {
      int64_t idx[U];
      int32_t j[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        idx[u] = base + (int64_t)(k0 + u < len ? k0 + u : k0) * 64;
        j[u] = k0 + u < len ? op.s_col[idx[u]] : 0;
      }
      uint8_t c[U];
#pragma unroll
      for (int u = 0; u < U; ++u) c[u] = k0 + u < len && j[u] >= op.nf ? code[j[u]] : 3;
      double dj[U][3];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t kk = j[u] >= op.nf ? (int64_t)j[u] - op.nf : 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) dj[u][a] = fd[3 * kk + a];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (c[u] != 3) {
          double v[6], pk[3];
#pragma unroll
          for (int q = 0; q < 6; ++q) v[q] = op.val[(int64_t)q * G + idx[u]];
          grip_of(dj[u], c[u], dy_top, dy_bot, pk);
          grip_mac(v, pk, k3);
        }
      }
    }
    load_rhs(ld, lr, dy_top, k3, b);
    return;
  }
  if constexpr (std::is_same<GM, GripVec>::value) {
    double k3[3] = {0.0, 0.0, 0.0};
    constexpr int U = 4;
    for (int k0 = 0; k0 < len; k0 += U) {
      int64_t idx[U];
      int32_t j[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        idx[u] = base + (int64_t)(k0 + u < len ? k0 + u : k0) * 64;
        j[u] = k0 + u < len ? op.s_col[idx[u]] : 0;
      }
      uint8_t c[U];
#pragma unroll
      for (int u = 0; u < U; ++u) c[u] = k0 + u < len && j[u] >= op.nf ? code[j[u]] : 3;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (c[u] != 3) {
          double v[6], pk[3];
#pragma unroll
          for (int q = 0; q < 6; ++q) v[q] = op.val[(int64_t)q * G + idx[u]];
          grip_of(*p, c[u], pk);
          grip_mac(v, pk, k3);
        }
      }
    }
    load_rhs(ld, lr, dy_top, k3, b);
    return;
  }
  constexpr int U = 4;
  for (int k0 = 0; k0 < len; k0 += U) {
    int64_t idx[U];
    int32_t j[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      idx[u] = base + (int64_t)(k0 + u < len ? k0 + u : k0) * 64;
      j[u] = k0 + u < len ? op.s_col[idx[u]] : 0;
    }
    uint8_t c[U];
#pragma unroll
    for (int u = 0; u < U; ++u) c[u] = k0 + u < len && j[u] >= op.nf ? code[j[u]] : 3;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (c[u] != 3) {  // a known neighbour (3: free or ghost free row, x₀ = 0)
        const double dy = c[u] == 2 ? dy_bot : dy_top;
        kx = fma(op.val[1 * G + idx[u]], dy, kx);
        ky = fma(op.val[3 * G + idx[u]], dy, ky);
        kz = fma(op.val[4 * G + idx[u]], dy, kz);
      }
    }
  }
  const double k3[3] = {kx, ky, kz};
  load_rhs(ld, lr, dy_top, k3, b);
}

// The CG's state at the start of a solve, from the reduced (‖b‖², ‖M⁻¹b‖²)
// (k_cg_init_finalize, cg.hip; the last block of k_amg_start, amg.hip)
__device__ __forceinline__ void cg_state_init(SolveState* st, double bb, double zz, double rtol, double atol,
                                              int norm, int max_it, double reg) {
  const double ref = norm == 1 ? zz : bb;
  const double t = rtol * rtol * ref, a2 = atol * atol;
  st->tol2 = t > a2 ? t : a2;
  st->rtol2 = rtol * rtol;
  st->atol2 = a2;
  st->reg = reg;
  st->bb0 = bb;
  st->res0 = ref;
  st->res_final = ref;
  st->base = 0;
  st->max_it = max_it;
  st->norm = norm;
  st->done = 0;
  st->iters = 0;
  st->status = 0;
  st->closed = 0;
}

// ---------------------------------------------------------------------------
// Shared pieces of the CG iteration kernels (cg.hip: SELL operator, ell.hip:
// wave-local lanes).
// ---------------------------------------------------------------------------
constexpr int kCgBS = 256;               // threads per block of the CG kernels
constexpr int kCgMaxG = kCgMaxPartials;  // max blocks (= partials re-read by each wave)

// y += V u with V the symmetric block (v0..v5)
__device__ __forceinline__ void block_mac(const double V[6], const double u[3], double y[3]) {
  y[0] = fma(V[0], u[0], fma(V[1], u[1], fma(V[2], u[2], y[0])));
  y[1] = fma(V[1], u[0], fma(V[3], u[1], fma(V[4], u[2], y[1])));
  y[2] = fma(V[2], u[0], fma(V[4], u[1], fma(V[5], u[2], y[2])));
}

template <bool BLOCK>
__device__ __forceinline__ void apply_m(const double* M, const double r[3], double u[3]) {
  if (BLOCK) {
    sym_apply(M, r, u);
  } else {
#pragma unroll
    for (int a = 0; a < 3; ++a) u[a] = M[a] * r[a];
  }
}

// ---------------------------------------------------------------------------
// Partial-sum protocol.  part = two parity buffers of [4][kCgMaxG] doubles.
// ---------------------------------------------------------------------------
__device__ __forceinline__ double* part_buf(double* part, int par) {
  return part + (size_t)par * 4 * kCgMaxG;
}

// Every lane ends with the grid total of the partials (block order, then a
// fixed butterfly): identical in every wave of every block.  PU = partial
// groups of 64 loaded per lane (G ≤ 64·PU).  The buffer is zeroed at the start
// of every solve and only blocks < G write it, so the slots ≥ G add exact
// zeros: every load is unconditional (a guarded or selected load makes hipcc
// branch and wait vmcnt(0) on all outstanding loads).
template <int PU>
__device__ __forceinline__ void wave_partials(const double* __restrict__ p, double s[4]) {
  const int lane = threadIdx.x & 63;
  double t[PU][4];
#pragma unroll
  for (int k = 0; k < PU; ++k) {
#pragma unroll
    for (int c = 0; c < 4; ++c) t[k][c] = p[c * kCgMaxG + lane + 64 * k];
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    double a = 0.0;
#pragma unroll
    for (int k = 0; k < PU; ++k) a += t[k][c];
    s[c] = wave_allsum(a);
  }
}

// block partial (thread 0 stores it; the next launch's waves re-reduce).
// The cross-wave step uses a raw s_barrier behind an LDS-only wait: a
// __syncthreads() would also wait for every outstanding vector store (vmcnt(0)).
template <int BS = kCgBS>
__device__ __forceinline__ void store_block_partial(double (&acc)[4], double* __restrict__ p) {
  constexpr int NW = BS / 64;
  __shared__ double lds[NW * 4];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = wave_allsum(acc[c]);
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c) lds[wid * 4 + c] = acc[c];
  }
  if (NW > 1) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if (threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      double s = lds[c];
      for (int w = 1; w < NW; ++w) s += lds[w * 4 + c];
      p[c * kCgMaxG + blockIdx.x] = s;
    }
  }
}

// α_j, β_j and the status of iteration j from the reduced partials S and the
// previous slot (identical in every wave of every block).
struct CgScalars {
  double alpha, beta, res;
  int status;
};
__device__ __forceinline__ CgScalars cg_scalars(const double S[4], int f0, double g0, double a0,
                                                double tol2, int it, int max_it, int norm) {
  CgScalars c;
  c.res = norm == 1 ? S[3] : S[2];
  const bool first = f0 == kInit;
  c.beta = first ? 0.0 : S[0] / g0;
  const double den = first ? S[1] : S[1] - c.beta * S[0] / a0;
  c.alpha = S[0] / den;
  if (f0 != kRun && f0 != kInit) c.status = kStop;
  else if (!(c.res > tol2)) c.status = isfinite(c.res) ? kConverged : kBreakdown;
  else if (it >= max_it) c.status = kMaxit;
  else c.status = ((den > 0.0) && isfinite(c.alpha) && isfinite(c.beta)) ? kRun : kBreakdown;
  return c;
}

// The closing check of a chunk (k_cg_advance, unpreconditioned norm): ‖r‖²
// of the chunk's last update from k_amg_rnorm's G block partials, summed as
// wave_partials<PU> sums the w kernel's (a lane's partials in block order,
// then the butterfly): the bits of S[2] in the update that would follow.
// Past G the select supplies the exact zeros that wave_partials reads from
// its zeroed buffer — this buffer is never zeroed.  One full wave.
__device__ __forceinline__ double cg_close_sum(const double* __restrict__ cpart, int G) {
  const int lane = threadIdx.x & 63;
  double a = 0.0;
#pragma unroll
  for (int k = 0; k < kCgMaxG / 64; ++k) {
    const int b = lane + 64 * k;
    a += b < G ? cpart[2 * kCgMaxG + b] : 0.0;
  }
  return wave_allsum(a);
}
// … and cg_scalars' convergence test on it.  Everything else that update
// could find (a non-finite norm, max_it, a breakdown) is left to it: the
// solve goes on and the update itself decides.
__device__ __forceinline__ bool cg_close_converged(double rr, double tol2) {
  return !(rr > tol2) && isfinite(rr);
}

// block 0 records iteration j's scalars in slots[j + 1]
__device__ __forceinline__ void cg_record(Slot* slots, int j, const double S[4],
                                          const CgScalars& c) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    Slot sl;
    sl.v[0] = S[0]; sl.v[1] = S[1]; sl.v[2] = S[2]; sl.v[3] = S[3];
    sl.alpha = c.alpha;
    sl.beta = c.beta;
    sl.res = c.res;
    sl.flag = c.status;
    sl.pad = 0;
    slots[j + 1] = sl;
  }
}

// TRACE: lane 0 of every wave records s_memrealtime (100 MHz) at entry, once
// the partials are reduced, once the last row's SpMV is done, and after its
// stores have drained: trace[(block·4 + wave)·4 + point] (diagnostics only).
template <bool TRACE, int BS = kCgBS>
__device__ __forceinline__ void trace_point(unsigned long long* trace, int point, double dep) {
  if (TRACE) {
    unsigned long long t;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : "v"(dep));
    if ((threadIdx.x & 63) == 0)
      trace[((size_t)blockIdx.x * (BS / 64) + (threadIdx.x >> 6)) * 4 + point] = t;
  }
}

}  // namespace mfea
