// kernels.hip — hand-written CDNA4 kernels of the mfea engine.  See kernels.hpp for
// the HBM layout and DESIGN.md for the roofline of each kernel.
//
// Compiled with -ffp-contract=off: the assembly and stress kernels restate the
// reference's rounding sequence (src/fea_solver.py:30-68, 260-272) and must not
// have products fused into adds behind our back.  The PCG kernels use explicit
// fma() where fusion is wanted.
#include "kernels.hpp"
#include "device_util.hpp"
#include "energy.hpp"

#include <math.h>

#include <type_traits>

namespace mfea {

// ---------------------------------------------------------------------------
// launch geometry
// ---------------------------------------------------------------------------
int64_t grid_rows(int64_t rows) { return rows <= 0 ? 0 : (rows + kBlock - 1) / kBlock; }
int64_t grid_elementwise(int64_t n) {
  int64_t g = (n + kBlock - 1) / kBlock;
  return g < 1 ? 1 : (g > 2048 ? 2048 : g);  // ≥ 8 blocks per CU, grid-stride beyond
}


// ---------------------------------------------------------------------------
// Element stiffness S_e (the 3×3 block of Ke = [[S,−S],[−S,S]]),
// src/fea_solver.py:30-68 / src/fea_petsc.cpp:88-140, same rounding sequence as
// the NumPy reference: L = √((vx²+vy²)+vz²), L_safe = max(L,1e-12), n = v/L_safe,
// k_ax = EA/L_safe, k_b = EI12/L_safe³, S_ab = (n_a n_b)·k_ax + (δ_ab − n_a n_b)·k_b.
// L_safe³ is formed in double-double (≈0.5 ulp; NumPy's pow is ≤1 ulp): cube,
// cube.hpp — shared with the element energy (energy.hpp).
// ---------------------------------------------------------------------------
// the section (EA, EI12) of element e: the handle's, or the element's own pair
__device__ __forceinline__ double2 section_of(const Material& m, int64_t) { return make_double2(m.EA, m.EI12); }
__device__ __forceinline__ double2 section_of(const ElemSection& m, int64_t e) { return m.sec[e]; }

__device__ __forceinline__ void bar_block(double vx, double vy, double vz, double EA, double EI12,
                                          double S[6], double* Lout) {
  const double L = sqrt(vx * vx + vy * vy + vz * vz);
  const double Ls = L < 1e-12 ? 1e-12 : L;
  const double n0 = vx / Ls, n1 = vy / Ls, n2 = vz / Ls;
  const double kax = EA / Ls;
  const double kb = EI12 / cube(Ls);
  const double t00 = n0 * n0, t01 = n0 * n1, t02 = n0 * n2, t11 = n1 * n1, t12 = n1 * n2,
               t22 = n2 * n2;
  S[0] = t00 * kax + (1.0 - t00) * kb;
  S[1] = t01 * kax + (0.0 - t01) * kb;
  S[2] = t02 * kax + (0.0 - t02) * kb;
  S[3] = t11 * kax + (1.0 - t11) * kb;
  S[4] = t12 * kax + (0.0 - t12) * kb;
  S[5] = t22 * kax + (1.0 - t22) * kb;
  if (Lout) *Lout = L;
}

// ---------------------------------------------------------------------------
// Assembly: owner-computes gather into the SELL-64 pattern.  One thread per
// node row; each slot (incident element) recomputes S_e from the two endpoint
// coordinates, writes −S_e (or 0 for an inactive element) with a fully
// coalesced SoA store, and accumulates the diagonal block in element order
// (= scipy's duplicate-summation order, src/fea_solver.py:105).  No atomics,
// no colouring, one launch, bitwise deterministic.
// ---------------------------------------------------------------------------
// One node row of the assembly; q (a free row of the GAMG solves): also
// K_fk x_k into k3 — k_amg_rhs's sum of the stored −S_e terms in slot order,
// the same bits.
// M: Material (one section for every element) or ElemSection (per-element
// (EA_e, EI12_e) pairs, kernels.hpp) — a template, not a run-time choice: a
// selected load would serialise the batch's gathers (below), and the uniform
// instantiation is the code it was before the pairs existed.
// GM: GripY, or GripVec with gp the launch's two prescribed displacements — a
// known neighbour's whole block then (grip_mac), the class still from the row
// position and inside the batch as before.
// GM = GripField (q->field): the same with p per neighbour, amplitude by the
// class.  The neighbour's vector is three more loads of the batch's second
// group, unconditional like the rest: on the index clamped to the first known
// row when the neighbour is free, the class applied afterwards.
template <class M, class GM = GripY>
__device__ __forceinline__ void assemble_row(int64_t N, int64_t row, const double* __restrict__ xyz,
                                             const int32_t* __restrict__ slice_ptr,
                                             const int32_t* __restrict__ row_len,
                                             const int32_t* __restrict__ s_col,
                                             const int32_t* __restrict__ s_elem,
                                             const uint8_t* __restrict__ active, const M& m,
                                             int64_t G, double* __restrict__ val, double* __restrict__ diag,
                                             const AsmRhs* q, double* k3, const GripP* gp = nullptr) {
  constexpr bool PE = !std::is_same<M, Material>::value;
  constexpr bool FLD = std::is_same<GM, GripField>::value;
  const bool rhs = q != nullptr && row < q->nf;
  const int64_t base = (int64_t)slice_ptr[row >> 6] * 64 + (row & 63);
  const int len = row_len[row];
  const double xi = xyz[3 * row], yi = xyz[3 * row + 1], zi = xyz[3 * row + 2];
  double d[6] = {0, 0, 0, 0, 0, 0};
  // slots in batches of U, each batch's loads issued together (slot → element
  // and column, then activity and coordinates): two dependent round trips per
  // batch instead of two per slot; the sums stay in slot order
  constexpr int U = 4;
  for (int k0 = 0; k0 < len; k0 += U) {
    // every load unconditional (a slot past the row's end re-reads its
    // batch's first slot, k0 < len), the masks applied after: a guarded or
    // selected load made hipcc branch per slot and wait vmcnt(0) in each
    // branch — the batch's gathers had run one slot at a time
    int64_t idx[U];
    int32_t e[U], j[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      ok[u] = k0 + u < len;
      idx[u] = base + (int64_t)(ok[u] ? k0 + u : k0) * 64;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      e[u] = s_elem[idx[u]];
      j[u] = s_col[idx[u]];
    }
    uint8_t act[U], cd[U];
    double pj[U][3];
    // per-element section: the slot's (EA_e, EI12_e) pair, one 16-byte load by
    // the element id the batch already holds — issued in this second group
    // with the activity and the coordinates, so the batch still waits for two
    // dependent round trips, not three
    double2 se[PE ? U : 1];
    double dj[FLD ? U : 1][3];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if constexpr (PE) se[u] = section_of(m, e[u]);
      if constexpr (FLD) {
        const int64_t kk = j[u] >= q->nf ? (int64_t)j[u] - q->nf : 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) dj[u][a] = q->field[3 * kk + a];
      }
      const uint8_t av = active[e[u]];
      act[u] = ok[u] ? av : 0;
      // the neighbour's class from its row position (no load: a select on a
      // loaded code made codegen branch around the load and wait in it)
      cd[u] = rhs && ok[u] && j[u] >= q->nf ? (j[u] < q->top_end ? 1 : j[u] < q->bot_end ? 2 : 3) : 3;
#pragma unroll
      for (int a = 0; a < 3; ++a) pj[u][a] = xyz[3 * (int64_t)j[u] + a];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (k0 + u >= len) break;
      double S[6] = {0, 0, 0, 0, 0, 0};
      if (act[u]) {
        // v = p2 − p1 with the row as either endpoint: the sign of v does not
        // change any product n_a n_b, so S is bitwise endpoint-symmetric.
        if constexpr (PE) bar_block(pj[u][0] - xi, pj[u][1] - yi, pj[u][2] - zi, se[u].x, se[u].y, S, nullptr);
        else bar_block(pj[u][0] - xi, pj[u][1] - yi, pj[u][2] - zi, m.EA, m.EI12, S, nullptr);
#pragma unroll
        for (int c = 0; c < 6; ++c) d[c] += S[c];
      }
      double v[6];
#pragma unroll
      for (int c = 0; c < 6; ++c) v[c] = -S[c];
#pragma unroll
      for (int c = 0; c < 6; ++c) val[(int64_t)c * G + idx[u]] = v[c];
      if (cd[u] != 3) {  // a known neighbour (3: free or ghost free row, x₀ = 0)
        if constexpr (std::is_same<GM, GripVec>::value) {
          double pk[3];
          grip_of(*gp, cd[u], pk);
          grip_mac(v, pk, k3);
        } else if constexpr (FLD) {
          double pk[3];
          grip_of(dj[u], cd[u], q->dy_top, q->dy_bot, pk);
          grip_mac(v, pk, k3);
        } else {
          const double dy = cd[u] == 2 ? q->dy_bot : q->dy_top;
          k3[0] = fma(v[1], dy, k3[0]);
          k3[1] = fma(v[3], dy, k3[1]);
          k3[2] = fma(v[4], dy, k3[2]);
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) diag[(int64_t)c * N + row] = d[c];
}

// ---------------------------------------------------------------------------
// Assembly, element-centric (option "asm_kernel" 1; north_star's "one
// wavefront per element batch … colour-partitioned writes"): one lane per
// element of a 64-element batch of ONE colour (symbolic.hpp ElemColour).
// S_e — the bar's BᵀDB, which for this element is k_ax nnᵀ + k_b (I − nnᵀ):
// six values — is formed ONCE per element in registers (the row gather forms
// it twice, once per endpoint row), −S_e goes to the element's slot in each
// endpoint row, and +S_e is added to both rows' diagonal blocks: no two
// elements of a colour share a node, so the colour's launch adds without
// atomics, and the colours run in order — deterministic.  Same S bits as the
// row gather (bar_block is endpoint-symmetric); the diagonal sums run in
// colour order instead of slot order (within a few ulps).  diag is zeroed
// before the first colour.
// ---------------------------------------------------------------------------
template <class M>
__global__ __launch_bounds__(kBlock) void k_assemble_colour(int64_t e0, int64_t e1, const int32_t* __restrict__ entry,
                                                            const int32_t* __restrict__ e2n,
                                                            const int32_t* __restrict__ epos,
                                                            const double* __restrict__ xyz,
                                                            const uint8_t* __restrict__ active, M m,
                                                            int64_t G, int64_t N, double* __restrict__ val,
                                                            double* __restrict__ diag) {
  const int64_t k = e0 + (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= e1) return;
  const int32_t e = entry[k];
  if (e < 0) return;
  const int32_t a = e2n[2 * e], b = e2n[2 * e + 1];
  const int32_t pa = epos[2 * e], pb = epos[2 * e + 1];
  double S[6] = {0, 0, 0, 0, 0, 0};
  if (active[e]) {
    const double2 se = section_of(m, e);
    bar_block(xyz[3 * (int64_t)b] - xyz[3 * (int64_t)a], xyz[3 * (int64_t)b + 1] - xyz[3 * (int64_t)a + 1],
              xyz[3 * (int64_t)b + 2] - xyz[3 * (int64_t)a + 2], se.x, se.y, S, nullptr);
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    val[(int64_t)c * G + pa] = -S[c];
    val[(int64_t)c * G + pb] = -S[c];
  }
  double da[6], db[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    da[c] = diag[(int64_t)c * N + a];
    db[c] = diag[(int64_t)c * N + b];
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    diag[(int64_t)c * N + a] = da[c] + S[c];
    diag[(int64_t)c * N + b] = db[c] + S[c];
  }
}

// Assembly, element pass + row pass (option "asm_kernel" 2): one lane per
// element forms S_e once and writes −S_e to its two slots (no two elements
// share a slot: no conflicts, no colours, one launch); then one lane per row
// sums −val over its slots in slot order into the diagonal block — the row
// gather's own order, so K is bit for bit the row gather's.
template <class M>
__global__ __launch_bounds__(kBlock) void k_assemble_elems(int64_t E, const int32_t* __restrict__ e2n,
                                                           const int32_t* __restrict__ epos,
                                                           const double* __restrict__ xyz,
                                                           const uint8_t* __restrict__ active, M m,
                                                           int64_t G, double* __restrict__ val) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= E) return;
  const int32_t pa = epos[2 * e], pb = epos[2 * e + 1];
  if (pa < 0) return;
  const int32_t a = e2n[2 * e], b = e2n[2 * e + 1];
  double S[6] = {0, 0, 0, 0, 0, 0};
  if (active[e]) {
    const double2 se = section_of(m, e);
    bar_block(xyz[3 * (int64_t)b] - xyz[3 * (int64_t)a], xyz[3 * (int64_t)b + 1] - xyz[3 * (int64_t)a + 1],
              xyz[3 * (int64_t)b + 2] - xyz[3 * (int64_t)a + 2], se.x, se.y, S, nullptr);
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    val[(int64_t)c * G + pa] = -S[c];
    val[(int64_t)c * G + pb] = -S[c];
  }
}

__global__ __launch_bounds__(kBlock) void k_diag_rows(int64_t N, const int32_t* __restrict__ slice_ptr,
                                                      const int32_t* __restrict__ row_len, int64_t G,
                                                      const double* __restrict__ val, double* __restrict__ diag) {
  const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (row >= N) return;
  const int64_t base = (int64_t)slice_ptr[row >> 6] * 64 + (row & 63);
  const int len = row_len[row];
  double d[6] = {0, 0, 0, 0, 0, 0};
  for (int k = 0; k < len; ++k) {
#pragma unroll
    for (int c = 0; c < 6; ++c) d[c] += -val[(int64_t)c * G + base + (int64_t)k * 64];
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) diag[(int64_t)c * N + row] = d[c];
}

// RHS: the GAMG solves' RHS too (AsmRhs: k_amg_rhs's outputs from the −S_e
// blocks in registers) — one launch fewer per step
// LD = NodeLoad (q.load): b = q − k; the row's load and mask byte are fetched
// in front of the row pass, with its slot pointer, length and coordinates, on
// the row clamped into the free rows (a known row reads row 0 and drops it).
template <bool RHS, class M, class GM = GripY, class LD = LoadNone>
__global__ __launch_bounds__(kBlock) void k_assemble(int64_t N, const double* __restrict__ xyz,
                                                     const int32_t* __restrict__ slice_ptr,
                                                     const int32_t* __restrict__ row_len,
                                                     const int32_t* __restrict__ s_col,
                                                     const int32_t* __restrict__ s_elem,
                                                     const uint8_t* __restrict__ active,
                                                     M m, int64_t G, double* __restrict__ val,
                                                     double* __restrict__ diag, AsmRhs q) {
  const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if constexpr (RHS) {
    if (q.dyp) {
      q.dy_top = q.dyp[0];
      q.dy_bot = q.dyp[1];
    }
    constexpr bool VEC = std::is_same<GM, GripVec>::value;
    GripP gp{};
    if constexpr (VEC) gp = grip_disp(q.grip, q.dy_top, q.dy_bot);
    double acc[2] = {0.0, 0.0};
    if (row < N) {
      double k3[3] = {0.0, 0.0, 0.0};
      LD ld{};
      if constexpr (std::is_same<LD, NodeLoad>::value) ld = q.load;
      const LoadRow<LD> lr = load_fetch(ld, row < q.nf ? row : 0);
      assemble_row<M, GM>(N, row, xyz, slice_ptr, row_len, s_col, s_elem, active, m, G, val, diag, &q, k3, &gp);
      if (row < q.nf) {
        double b[3];
        load_rhs(ld, lr, q.dy_top, k3, b);
#pragma unroll
        for (int a = 0; a < 3; ++a) q.r[3 * row + a] = b[a];
#pragma unroll
        for (int a = 0; a < 3; ++a) acc[0] = fma(b[a], b[a], acc[0]);
      } else {
        const uint8_t c = q.code[row];
        double xk[3] = {0.0, c == 3 ? 0.0 : (c == 2 ? q.dy_bot : q.dy_top), 0.0};
        if constexpr (VEC) grip_of(gp, c, xk);
        if constexpr (std::is_same<GM, GripField>::value)
          grip_of(GripField{q.field}, row, q.nf, c, q.dy_top, q.dy_bot, xk);
#pragma unroll
        for (int a = 0; a < 3; ++a) q.x[3 * row + a] = xk[a];
      }
    }
    block_publish<2>(acc, q.partials, q.ticket, q.red_out);
  } else {
    if (row < N) assemble_row(N, row, xyz, slice_ptr, row_len, s_col, s_elem, active, m, G, val, diag, nullptr, nullptr);
  }
}

__global__ void k_init_finalize(const double* red, double rtol, double atol, int norm, int max_it,
                                double reg, Slot* slots, SolveState* st) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double rz = red[0], bb = red[1], zz = red[2];
  const double ref = norm == 1 ? zz : bb;
  const double t = rtol * rtol * ref, a2 = atol * atol;
  st->tol2 = t > a2 ? t : a2;
  st->reg = reg;
  st->bb0 = bb;
  st->res_final = ref;
  st->res0 = ref;
  st->base = 0;
  st->max_it = max_it;
  st->norm = norm;
  st->done = 0;
  st->iters = 0;
  st->status = 0;
  Slot s0;
  s0.v[0] = 0.0; s0.v[1] = rz; s0.v[2] = bb; s0.v[3] = zz;
  s0.flag = kRun;
  slots[0] = s0;
}

// run(j): iteration base+j executes.  Pure function of globally reduced values,
// so every block (and, multi-GPU, every rank) agrees.
__device__ __forceinline__ bool run_iter(const Slot* slots, const SolveState* st, int j) {
  const Slot& s = slots[j];
  const double res = st->norm == 1 ? s.v[3] : s.v[2];
  return s.flag == kRun && res > st->tol2 && (st->base + j) < st->max_it;
}

// ---------------------------------------------------------------------------
// x += α p ; r −= α q ; z = M⁻¹ r ; reduce (r·z, r·r, z·z) into slot j+1.
// ---------------------------------------------------------------------------
template <bool BLOCK>
__global__ __launch_bounds__(kBlock) void k_update(int j, int64_t n, double* __restrict__ x,
                                                   double* __restrict__ r,
                                                   const double* __restrict__ p,
                                                   const double* __restrict__ q,
                                                   const double* __restrict__ dinv, Slot* slots,
                                                   const SolveState* st, double* partials,
                                                   unsigned* ticket) {
  if (!run_iter(slots, st, j)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) slots[j + 1].flag = kStop;
    return;
  }
  const double pq = slots[j].v[0];
  const double alpha = slots[j].v[1] / pq;
  if (!(pq > 0.0) || !isfinite(alpha)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      slots[j + 1].v[1] = 0.0; slots[j + 1].v[2] = 0.0; slots[j + 1].v[3] = 0.0;
      slots[j + 1].flag = kBreakdown;
    }
    return;
  }
  double acc[3] = {0.0, 0.0, 0.0};
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  if (!BLOCK) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
      x[i] = fma(alpha, p[i], x[i]);
      const double ri = fma(-alpha, q[i], r[i]);
      r[i] = ri;
      const double zi = dinv[i] * ri;
      acc[0] = fma(ri, zi, acc[0]);
      acc[1] = fma(ri, ri, acc[1]);
      acc[2] = fma(zi, zi, acc[2]);
    }
  } else {
    for (int64_t nd = (int64_t)blockIdx.x * kBlock + threadIdx.x; nd < n / 3; nd += stride) {
      double rv[3], zv[3], B[6];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const int64_t i = 3 * nd + a;
        x[i] = fma(alpha, p[i], x[i]);
        rv[a] = fma(-alpha, q[i], r[i]);
        r[i] = rv[a];
      }
#pragma unroll
      for (int c = 0; c < 6; ++c) B[c] = dinv[6 * nd + c];
      sym_apply(B, rv, zv);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        acc[0] = fma(rv[a], zv[a], acc[0]);
        acc[1] = fma(rv[a], rv[a], acc[1]);
        acc[2] = fma(zv[a], zv[a], acc[2]);
      }
    }
  }
  if (block_publish<3>(acc, partials, ticket, &slots[j + 1].v[1]) && threadIdx.x == 0)
    slots[j + 1].flag = kRun;
}

// p = M⁻¹ r + β p, β = (r·z)_{j+1} / (r·z)_j — only if iteration j+1 will run.
template <bool BLOCK>
__global__ __launch_bounds__(kBlock) void k_direction(int j, int64_t n, const double* __restrict__ r,
                                                      double* __restrict__ p,
                                                      const double* __restrict__ dinv,
                                                      const Slot* slots, const SolveState* st) {
  if (!run_iter(slots, st, j + 1)) return;
  const double beta = slots[j + 1].v[1] / slots[j].v[1];
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  if (!BLOCK) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride)
      p[i] = fma(beta, p[i], dinv[i] * r[i]);
  } else {
    for (int64_t nd = (int64_t)blockIdx.x * kBlock + threadIdx.x; nd < n / 3; nd += stride) {
      double rv[3], zv[3], B[6];
#pragma unroll
      for (int a = 0; a < 3; ++a) rv[a] = r[3 * nd + a];
#pragma unroll
      for (int c = 0; c < 6; ++c) B[c] = dinv[6 * nd + c];
      sym_apply(B, rv, zv);
#pragma unroll
      for (int a = 0; a < 3; ++a) p[3 * nd + a] = fma(beta, p[3 * nd + a], zv[a]);
    }
  }
}

// End of a chunk of `chunk` iterations: record the stop point or roll slot
// `chunk` into slot 0.  Once done, slot 0 is poisoned STOP so any chunk the
// host has already queued is a no-op.
__global__ void k_advance(int chunk, Slot* slots, SolveState* st) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (st->done) return;
  for (int j = 0; j <= chunk; ++j) {
    if (!run_iter(slots, st, j)) {
      const Slot& s = slots[j];
      const double res = st->norm == 1 ? s.v[3] : s.v[2];
      st->iters = st->base + j;
      st->res_final = res;
      if (s.flag == kBreakdown) st->status = -5;
      else if (s.flag == kRun && res <= st->tol2) st->status = 0;
      else if (s.flag == kRun) st->status = -4;
      else st->status = -5;  // kStop without a recorded reason cannot happen
      st->done = 1;
      slots[0].flag = kStop;
      return;
    }
  }
  slots[0] = slots[chunk];
  st->base += chunk;
}

// ---------------------------------------------------------------------------
// Reaction: Σ over top grip rows of (K·U)_y with the unregularised K
// (src/fea_solver.py:252-254, src/fea_petsc.cpp:360-372).  Top rows are a
// contiguous range of the permutation.
// GM = GripVec: the reaction vector — all three rows of every block in the
// same slot order (reaction_row3), three sums through one publish into `sums`,
// and the work-conjugate force along g.top into red_out (NULL: the sums alone;
// the bottom band of mfea_get_reaction), formed by the block that ends the
// reduction: F = (t₀·S₀ + t₁·S₁) + t₂·S₂.
// GM = GripField (g.d: the vector of row row0, the band's first): the same
// row body, then the row's generalised force w = (d₀·f₀ + d₁·f₁) + d₂·f₂ — one
// sum through the tensile reaction's publish into red_out.
// ---------------------------------------------------------------------------
template <class GM>
__global__ __launch_bounds__(kBlock) void k_reaction(int64_t row0, int64_t nrows, int64_t N,
                                                     const int32_t* __restrict__ slice_ptr,
                                                     const int32_t* __restrict__ row_len,
                                                     const int32_t* __restrict__ s_col,
                                                     const double* __restrict__ val,
                                                     const double* __restrict__ diag, int64_t G,
                                                     const double* __restrict__ u, double* partials,
                                                     unsigned* ticket, double* red_out, GM g, double* sums) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if constexpr (std::is_same<GM, GripVec>::value) {
    double f3[3] = {0.0, 0.0, 0.0};
    if (t < nrows) reaction_row3(row0 + t, N, slice_ptr, row_len, s_col, val, diag, G, u, f3);
    reaction3_publish(f3, partials, ticket, sums, g.top, red_out, gridDim.x, blockIdx.x);
    return;
  }
  if constexpr (std::is_same<GM, GripField>::value) {
    double w[1] = {0.0};
    if (t < nrows) {
      double f3[3];
      reaction_row3(row0 + t, N, slice_ptr, row_len, s_col, val, diag, G, u, f3);
      w[0] = grip_work_row(g.d + 3 * t, f3);
    }
    block_publish<1>(w, partials, ticket, red_out);
    return;
  }
  double f[1] = {0.0};
  if (t < nrows) {
    const int64_t row = row0 + t;
    const int64_t base = (int64_t)slice_ptr[row >> 6] * 64 + (row & 63);
    const int len = row_len[row];
    double fy = diag[N + row] * u[3 * row] + diag[3 * N + row] * u[3 * row + 1] +
                diag[4 * N + row] * u[3 * row + 2];
    // slots in batches of four, each batch's columns and values issued before
    // its gathers (one latency chain per batch, not per slot); the padding
    // lanes of a batch re-read slot k0 and add nothing.  Terms in slot order.
    constexpr int U = 4;
    for (int k0 = 0; k0 < len; k0 += U) {
      int64_t idx[U], c[U];
#pragma unroll
      for (int q = 0; q < U; ++q) {
        idx[q] = base + (int64_t)(k0 + q < len ? k0 + q : k0) * 64;
        c[q] = s_col[idx[q]];
      }
      double t[U];
#pragma unroll
      for (int q = 0; q < U; ++q)
        t[q] = val[G + idx[q]] * u[3 * c[q]] + val[3 * G + idx[q]] * u[3 * c[q] + 1] +
               val[4 * G + idx[q]] * u[3 * c[q] + 2];
#pragma unroll
      for (int q = 0; q < U; ++q)
        if (k0 + q < len) fy += t[q];
    }
    f[0] = fy;
  }
  block_publish<1>(f, partials, ticket, red_out);
}

// ---------------------------------------------------------------------------
// The work of the nodal loads (mfea_get_load_work): one lane per free row,
// L_r = (q[0]·u[0] + q[1]·u[1]) + q[2]·u[2] with q as the RHS kernels form it
// (0 on a floating row), f64, nothing fused; k_reaction's publish, so the rows
// reduce in its fixed order.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_load_work(int64_t nf, NodeLoad ld, double dy_top,
                                                      const double* __restrict__ u, double* partials,
                                                      unsigned* ticket, double* red_out) {
  const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  double w[1] = {0.0};
  if (row < nf) {
    const LoadRow<NodeLoad> lr = load_fetch(ld, row);
    const double ur[3] = {u[3 * row], u[3 * row + 1], u[3 * row + 2]};
    double q[3];
    load_q(ld, lr, dy_top, q);
    w[0] = grip_work_row(q, ur);
  }
  block_publish<1>(w, partials, ticket, red_out);
}

// ---------------------------------------------------------------------------
// Stress / failure, src/fea_solver.py:259-274: for elements active at step
// start, ε = (n·(u2−u1))/L with n = v/L (no L clamp in Python), the dot product
// as BLAS ddot forms it (fma chain x0y0 → +x1y1 → +x2y2), σ = E·ε, deactivate
// if |ε| > max_strain.  Inactive elements record σ = 0.  Reduces #active.
// ---------------------------------------------------------------------------
// M: Material, or ElemPost — E_e and max_strain_e read at e (coalesced), each
// falling back to the scalar where its array is absent.
__device__ __forceinline__ double modulus_of(const Material& m, int64_t) { return m.E; }
__device__ __forceinline__ double modulus_of(const ElemPost& m, int64_t e) { return m.Ee ? m.Ee[e] : m.E; }
__device__ __forceinline__ double strength_of(const Material&, int64_t, double s) { return s; }
__device__ __forceinline__ double strength_of(const ElemPost& m, int64_t e, double s) {
  return m.strength ? m.strength[e] : s;
}

template <class M>
__global__ __launch_bounds__(kBlock) void k_stress(int64_t E, const int32_t* __restrict__ e2n,
                                                   const double* __restrict__ xyz,
                                                   const double* __restrict__ u, M m,
                                                   double max_strain, uint8_t* __restrict__ active,
                                                   double* __restrict__ stress, double* partials,
                                                   unsigned* ticket, double* red_out,
                                                   const uint8_t* __restrict__ owned,
                                                   int32_t* __restrict__ fail_list, unsigned* fail_cnt) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  double cnt[1] = {0.0};
  if (e < E) {
    const int32_t a = e2n[2 * e], b = e2n[2 * e + 1];
    const uint8_t act0 = active[e];
    uint8_t act = act0;
    double sg = 0.0;
    if (act && a >= 0) {
      const double vx = xyz[3 * b] - xyz[3 * a], vy = xyz[3 * b + 1] - xyz[3 * a + 1],
                   vz = xyz[3 * b + 2] - xyz[3 * a + 2];
      // np.linalg.norm of one 3-vector = sqrt(v·v) through BLAS ddot (py:266)
      const double L = sqrt(fma(vz, vz, fma(vy, vy, vx * vx)));
      const double n0 = vx / L, n1 = vy / L, n2 = vz / L;
      const double du0 = u[3 * b] - u[3 * a], du1 = u[3 * b + 1] - u[3 * a + 1],
                   du2 = u[3 * b + 2] - u[3 * a + 2];
      const double dot = fma(n2, du2, fma(n1, du1, n0 * du0));
      const double strain = dot / L;
      sg = modulus_of(m, e) * strain;
      if (fabs(strain) > strength_of(m, e, max_strain)) act = 0;
      active[e] = act;
    }
    stress[e] = sg;
    cnt[0] = (act && (!owned || owned[e])) ? 1.0 : 0.0;
    // an (owned) element failing now joins the list (any order): the host's
    // activity then moves by these ids instead of an E-byte copy or reduction
    // (capi.hip post_impl / apply_failures)
    if (fail_list && act0 && !act && (!owned || owned[e])) fail_list[atomicAdd(fail_cnt, 1u)] = (int32_t)e;
  }
  block_publish<1>(cnt, partials, ticket, red_out);
}

// Undo a post's failures (capi.hip spec_undo): the elements k_stress listed
// are active again and the list's counter is zero — a post enqueued behind a
// CG batch that turned out not to be the last one leaves no trace
__global__ __launch_bounds__(kBlock) void k_unfail(const int32_t* __restrict__ fail_list, unsigned* cnt,
                                                   uint8_t* __restrict__ active) {
  const unsigned c = *cnt;
  for (unsigned k = threadIdx.x; k < c; k += kBlock) active[fail_list[k]] = 1;
  __syncthreads();
  if (threadIdx.x == 0) *cnt = 0u;
}

// ---------------------------------------------------------------------------
// Strain energy per element (mfea_get_energy; energy.hpp holds the arithmetic
// and its operation order): one lane per element, w_ax / w_b / g_ax / g_b of
// an element that counts — active in the mask given, both endpoints kept —
// and four zeros otherwise.  Each output array is written only where it was
// asked for (a uniform branch on a kernel argument).  Reduces (Σ w_ax, Σ w_b)
// through block_publish: block order, then shard order — the same bits on
// every call.  Nothing is written but the outputs.
// Loads: the endpoints, the activity byte and (M = ElemSection) the section
// pair are indexed by e and issued together; the twelve gathers they lead to
// (coordinates and displacements of both nodes) are all issued before the
// first use, as k_stress issues its own — two dependent round trips a lane.
// ---------------------------------------------------------------------------
template <class M>
__global__ __launch_bounds__(kBlock) void k_energy(int64_t E, const int32_t* __restrict__ e2n,
                                                   const double* __restrict__ xyz,
                                                   const double* __restrict__ u,
                                                   const uint8_t* __restrict__ active, M m, EnergyOut out,
                                                   double* partials, unsigned* ticket, double* red_out) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  double acc[2] = {0.0, 0.0};
  if (e < E) {
    const int32_t a = e2n[2 * e], b = e2n[2 * e + 1];
    const uint8_t act = active[e];
    const double2 se = section_of(m, e);
    ElemEnergy r{0.0, 0.0, 0.0, 0.0};
    if (act && a >= 0 && b >= 0) {
      const int64_t ia = 3 * (int64_t)a, ib = 3 * (int64_t)b;
      const double pa[3] = {xyz[ia], xyz[ia + 1], xyz[ia + 2]}, pb[3] = {xyz[ib], xyz[ib + 1], xyz[ib + 2]};
      const double ua[3] = {u[ia], u[ia + 1], u[ia + 2]}, ub[3] = {u[ib], u[ib + 1], u[ib + 2]};
      r = element_energy(pa, pb, ua, ub, se.x, se.y);
    }
    if (out.w_axial) out.w_axial[e] = r.w_ax;
    if (out.w_bending) out.w_bending[e] = r.w_b;
    if (out.g_axial) out.g_axial[e] = r.g_ax;
    if (out.g_bending) out.g_bending[e] = r.g_b;
    acc[0] = r.w_ax;
    acc[1] = r.w_b;
  }
  block_publish<2>(acc, partials, ticket, red_out);
}

// ---------------------------------------------------------------------------
// Floating free rows on the device: connected components of the active
// element graph, then per component whether a grip row is in it.  A free
// row of a component without a grip is floating: zero load, so the direct
// solve leaves it at exactly zero (src/fea_solver.py:128) and the kept GAMG
// hierarchy masks its P_0 row (capi.hip enqueue_fmask).  Replaces a host
// union-find over every element per new active set.
//
// The rows are in depth-first order of the free-node graph (symbolic.hpp):
// hyphal chains are runs of consecutive rows, so nearly every coupling joins
// two rows of the same 4096-row tile.  Pass 1 (one workgroup per tile) runs
// union-find over the tile's own couplings in LDS and links every row to its
// tile-local root; pass 2 hooks the few couplings between tiles into those
// roots with CAS in HBM; pass 3 flattens.  Roots only ever link under smaller
// rows, so every component ends at its smallest row whatever order the
// hooks ran in: the result is deterministic.
// ---------------------------------------------------------------------------
constexpr int kSlice = 64;  // SELL-64 rows per slice (symbolic.hpp)

__device__ __forceinline__ int32_t cc_load(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of v, halving the path behind it (a parent only ever moves to a
// smaller row of the same component, so a racing shortcut stays valid)
__device__ __forceinline__ int32_t cc_root(int32_t* parent, int32_t v) {
  int32_t cur = cc_load(parent + v);
  if (cur != v) {
    int32_t prev = v, next;
    while (cur > (next = cc_load(parent + cur))) {
      __hip_atomic_store(parent + prev, next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      prev = cur;
      cur = next;
    }
  }
  return cur;
}

__device__ __forceinline__ int32_t lds_root(volatile int32_t* lp, int32_t v) {
  int32_t cur = lp[v], next;
  if (cur != v) {
    int32_t prev = v;
    while (cur > (next = lp[cur])) {
      lp[prev] = next;
      prev = cur;
      cur = next;
    }
  }
  return cur;
}

// pass 1: union-find over the couplings inside one tile of rows, in LDS;
// parent[row] = its tile-local root (a global row), anchored[row] = 0
template <int kCcTile>
__global__ __launch_bounds__(kBlock) void k_cc_local(int64_t n, const int32_t* __restrict__ slice_ptr,
                                                     const int32_t* __restrict__ row_len,
                                                     const int32_t* __restrict__ s_col,
                                                     const int32_t* __restrict__ s_elem,
                                                     const uint8_t* __restrict__ active, int32_t* __restrict__ parent,
                                                     uint8_t* __restrict__ anchored) {
  __shared__ int32_t lp[kCcTile];
  const int64_t base = (int64_t)blockIdx.x * kCcTile;
  const int rows = (int)min<int64_t>(kCcTile, n - base);
  for (int i = threadIdx.x; i < rows; i += kBlock) lp[i] = i;
  __syncthreads();
  for (int i = threadIdx.x; i < rows; i += kBlock) {
    const int64_t r = base + i;
    const int len = row_len[r];
    const int64_t p0 = (int64_t)slice_ptr[r >> 6] * kSlice + (r & 63);
    for (int k = 0; k < len; ++k) {
      const int64_t pos = p0 + (int64_t)k * kSlice;
      const int32_t c = s_col[pos];
      const int64_t j = (int64_t)c - base;
      if (c < 0 || j <= i || j >= rows || !active[s_elem[pos]]) continue;
      int32_t a = lds_root(lp, i), b = lds_root(lp, (int32_t)j);
      while (a != b) {  // hook the larger root under the smaller
        if (a > b) {
          const int32_t t = a;
          a = b;
          b = t;
        }
        const int32_t old = atomicCAS(&lp[b], b, a);
        if (old == b) break;
        b = lds_root(lp, old);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < rows; i += kBlock) {
    int32_t c = lp[i], next;
    while (c > (next = lp[c])) c = next;
    parent[base + i] = (int32_t)(base + c);
    anchored[base + i] = 0;
  }
}

// pass 2: the couplings between tiles hook tile roots together (CAS in HBM)
__global__ __launch_bounds__(kBlock) void k_cc_cross(int64_t n, const int32_t* __restrict__ slice_ptr,
                                                     const int32_t* __restrict__ row_len,
                                                     const int32_t* __restrict__ s_col,
                                                     const int32_t* __restrict__ s_elem,
                                                     const uint8_t* __restrict__ active, int32_t* parent,
                                                     int tile_rows) {
  const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r >= n) return;
  const int len = row_len[r];
  const int64_t p0 = (int64_t)slice_ptr[r >> 6] * kSlice + (r & 63);
  const int64_t tile = r / tile_rows;
  for (int k = 0; k < len; ++k) {
    const int64_t pos = p0 + (int64_t)k * kSlice;
    const int32_t c = s_col[pos];
    if (c <= r || c / tile_rows == tile || !active[s_elem[pos]]) continue;
    int32_t a = cc_root(parent, (int32_t)r), b = cc_root(parent, c);
    while (a != b) {
      if (a > b) {
        const int32_t t = a;
        a = b;
        b = t;
      }
      const int32_t old = atomicCAS(parent + b, b, a);
      if (old == b) break;
      b = cc_root(parent, old);
    }
  }
}

// pass 3: every row's parent to its root (the walk writes nothing but the
// row's own link, so a concurrent walk reads either link — both lead to the
// root); grip rows [g0, g1) mark their root anchored
__global__ __launch_bounds__(kBlock) void k_cc_flatten(int64_t n, int32_t* parent, int64_t g0, int64_t g1,
                                                       uint8_t* __restrict__ anchored) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int32_t old = cc_load(parent + i);
  int32_t r = old, next;
  while (r > (next = cc_load(parent + r))) r = next;
  if (r != old) __hip_atomic_store(parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (i >= g0 && i < g1) anchored[r] = 1;
}

// mask[label[i]] = 1 iff free row i's component holds no grip row
__global__ __launch_bounds__(kBlock) void k_cc_mask(int64_t nf, const int32_t* __restrict__ parent,
                                                    const uint8_t* __restrict__ anchored,
                                                    const int32_t* __restrict__ label, uint8_t* __restrict__ mask) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= nf) return;
  mask[label ? label[i] : i] = anchored[parent[i]] ? 0 : 1;
}

__global__ __launch_bounds__(kBlock) void k_element_stiffness(int64_t n, const double* __restrict__ p1,
                                                              const double* __restrict__ p2,
                                                              Material m, double* __restrict__ Ke,
                                                              double* __restrict__ L) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= n) return;
  double S[6], l;
  bar_block(p2[3 * e] - p1[3 * e], p2[3 * e + 1] - p1[3 * e + 1], p2[3 * e + 2] - p1[3 * e + 2], m.EA,
            m.EI12, S, &l);
  L[e] = l;
  const int sidx[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
  for (int a = 0; a < 6; ++a)
    for (int b = 0; b < 6; ++b) {
      const double v = S[sidx[a % 3][b % 3]];
      Ke[36 * e + 6 * a + b] = ((a < 3) == (b < 3)) ? v : -v;
    }
}

// ---------------------------------------------------------------------------
// Generic scalar CSR operator for solve_system(K, known_dofs, known_vals)
// with a caller-supplied K (src/fea_solver.py:112-135).  Known DOFs keep
// dinv = 0, r = 0, p = 0, so the shared update/direction kernels run over all
// n DOFs unmasked and never move a prescribed value.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_csr_rhs_init(
    int64_t n, const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const double* __restrict__ data, const uint8_t* __restrict__ known, const double* __restrict__ kval,
    double reg, double* __restrict__ x, double* __restrict__ r, double* __restrict__ p,
    double* __restrict__ dinv, double* partials, unsigned* ticket, double* red_out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  double acc[3] = {0.0, 0.0, 0.0};
  if (i < n) {
    if (known[i]) {
      x[i] = kval[i]; r[i] = 0.0; p[i] = 0.0; dinv[i] = 0.0;
    } else {
      double kx = 0.0, dii = 0.0;
      for (int64_t t = indptr[i]; t < indptr[i + 1]; ++t) {
        const int32_t c = indices[t];
        if (known[c]) kx = fma(data[t], kval[c], kx);
        if (c == i) dii += data[t];
      }
      const double b = 0.0 - kx;
      const double d = 1.0 / (dii + reg);
      const double z = d * b;
      x[i] = 0.0; r[i] = b; p[i] = z; dinv[i] = d;
      acc[0] = b * z; acc[1] = b * b; acc[2] = z * z;
    }
  }
  block_publish<3>(acc, partials, ticket, red_out);
}

__global__ __launch_bounds__(kBlock) void k_spmv_csr(int j, int64_t n, const int64_t* __restrict__ indptr,
                                                     const int32_t* __restrict__ indices,
                                                     const double* __restrict__ data,
                                                     const uint8_t* __restrict__ known, double reg,
                                                     const double* __restrict__ p,
                                                     double* __restrict__ q, Slot* slots,
                                                     const SolveState* st, double* partials,
                                                     unsigned* ticket) {
  if (!run_iter(slots, st, j)) return;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  double pq[1] = {0.0};
  if (i < n) {
    double y = 0.0;
    if (!known[i]) {
      y = reg * p[i];
      for (int64_t t = indptr[i]; t < indptr[i + 1]; ++t) y = fma(data[t], p[indices[t]], y);
    }
    q[i] = y;
    pq[0] = p[i] * y;
  }
  block_publish<1>(pq, partials, ticket, &slots[j].v[0]);
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
#define MFEA_GRID(n) dim3((unsigned)(n)), dim3(kBlock), 0, s

// f(m) or f(ElemSection{sec}): the material form by the per-element array
template <class F>
static void with_material(Material m, const double2* sec, F&& f) {
  if (sec) f(ElemSection{sec});
  else f(m);
}

void launch_assemble(hipStream_t s, int64_t N, const double* xyz, const int32_t* slice_ptr,
                     const int32_t* row_len, const int32_t* s_col, const int32_t* s_elem,
                     const uint8_t* active, Material m, int64_t G, double* val, double* diag,
                     const AsmRhs* rhs, const double2* sec) {
  if (!rhs && N <= 0) return;  // (the RHS form's blocks publish their reduction even when N = 0)
  with_material(m, sec, [&](auto mm) {
    using M = decltype(mm);
    if (!rhs) {
      hipLaunchKernelGGL((k_assemble<false, M>), MFEA_GRID(grid_rows(N)), N, xyz, slice_ptr, row_len, s_col, s_elem,
                         active, mm, G, val, diag, AsmRhs{});
      return;
    }
    // the RHS form of the row gather: the grip and load forms by the fields of rhs
    const BcForm bc{rhs->vec ? &rhs->grip : nullptr, rhs->field, rhs->load.f ? &rhs->load : nullptr};
    with_bc(bc, [&](auto g, auto ld) {
      hipLaunchKernelGGL((k_assemble<true, M, decltype(g), decltype(ld)>), MFEA_GRID(grid_rows(N > 0 ? N : 1)), N,
                         xyz, slice_ptr, row_len, s_col, s_elem, active, mm, G, val, diag, *rhs);
    });
  });
}

void launch_assemble_colour(hipStream_t s, int colors, const int32_t* cstart, const int32_t* entry,
                            const int32_t* e2n, const int32_t* epos, const double* xyz, const uint8_t* active,
                            Material m, int64_t G, int64_t N, double* val, double* diag, const double2* sec) {
  if (N > 0) (void)hipMemsetAsync(diag, 0, (size_t)6 * N * sizeof(double), s);
  for (int c = 0; c < colors; ++c) {
    const int64_t e0 = cstart[c], e1 = cstart[c + 1];
    if (e1 <= e0) continue;
    if (sec)
      hipLaunchKernelGGL(k_assemble_colour<ElemSection>, MFEA_GRID(grid_rows(e1 - e0)), e0, e1, entry, e2n, epos, xyz,
                         active, ElemSection{sec}, G, N, val, diag);
    else
      hipLaunchKernelGGL(k_assemble_colour<Material>, MFEA_GRID(grid_rows(e1 - e0)), e0, e1, entry, e2n, epos, xyz,
                         active, m, G, N, val, diag);
  }
}

void launch_assemble_elems(hipStream_t s, int64_t E, int64_t N, const int32_t* e2n, const int32_t* epos,
                           const double* xyz, const uint8_t* active, Material m, const int32_t* slice_ptr,
                           const int32_t* row_len, int64_t G, double* val, double* diag, const double2* sec) {
  if (E > 0 && sec)
    hipLaunchKernelGGL(k_assemble_elems<ElemSection>, MFEA_GRID(grid_rows(E)), E, e2n, epos, xyz, active,
                       ElemSection{sec}, G, val);
  else if (E > 0)
    hipLaunchKernelGGL(k_assemble_elems<Material>, MFEA_GRID(grid_rows(E)), E, e2n, epos, xyz, active, m, G, val);
  if (N > 0) hipLaunchKernelGGL(k_diag_rows, MFEA_GRID(grid_rows(N)), N, slice_ptr, row_len, G, val, diag);
}

void launch_init_finalize(hipStream_t s, const double* red, double rtol, double atol, int norm,
                          int max_it, double reg, Slot* slots, SolveState* st) {
  hipLaunchKernelGGL(k_init_finalize, dim3(1), dim3(64), 0, s, red, rtol, atol, norm, max_it, reg,
                     slots, st);
}

void launch_update(hipStream_t s, int j, int64_t n, int precond, double* x, double* r,
                   const double* p, const double* q, const double* dinv, Slot* slots,
                   const SolveState* st, double* partials, unsigned* ticket) {
  if (precond == 1)
    hipLaunchKernelGGL(k_update<true>, MFEA_GRID(grid_elementwise(n / 3)), j, n, x, r, p, q, dinv,
                       slots, st, partials, ticket);
  else
    hipLaunchKernelGGL(k_update<false>, MFEA_GRID(grid_elementwise(n)), j, n, x, r, p, q, dinv,
                       slots, st, partials, ticket);
}

void launch_direction(hipStream_t s, int j, int64_t n, int precond, const double* r, double* p,
                      const double* dinv, const Slot* slots, const SolveState* st) {
  if (precond == 1)
    hipLaunchKernelGGL(k_direction<true>, MFEA_GRID(grid_elementwise(n / 3)), j, n, r, p, dinv,
                       slots, st);
  else
    hipLaunchKernelGGL(k_direction<false>, MFEA_GRID(grid_elementwise(n)), j, n, r, p, dinv, slots,
                       st);
}

void launch_advance(hipStream_t s, int chunk, Slot* slots, SolveState* st) {
  hipLaunchKernelGGL(k_advance, dim3(1), dim3(64), 0, s, chunk, slots, st);
}

void launch_reaction(hipStream_t s, int64_t row0, int64_t nrows, int64_t N,
                     const int32_t* slice_ptr, const int32_t* row_len, const int32_t* s_col,
                     const double* val, const double* diag, int64_t G, const double* u,
                     double* partials, unsigned* ticket, double* red_out) {
  hipLaunchKernelGGL(k_reaction<GripY>, MFEA_GRID(grid_rows(nrows > 0 ? nrows : 1)), row0, nrows, N,
                     slice_ptr, row_len, s_col, val, diag, G, u, partials, ticket, red_out, GripY{},
                     (double*)nullptr);
}

void launch_reaction3(hipStream_t s, int64_t row0, int64_t nrows, int64_t N, const int32_t* slice_ptr,
                      const int32_t* row_len, const int32_t* s_col, const double* val, const double* diag,
                      int64_t G, const double* u, double* partials, unsigned* ticket, double* sums,
                      const double* w, double* force_out) {
  GripVec g{};
  for (int c = 0; c < 3 && w; ++c) g.top[c] = w[c];
  hipLaunchKernelGGL(k_reaction<GripVec>, MFEA_GRID(grid_rows(nrows > 0 ? nrows : 1)), row0, nrows, N, slice_ptr,
                     row_len, s_col, val, diag, G, u, partials, ticket, w ? force_out : nullptr, g, sums);
}

void launch_reaction_field(hipStream_t s, int64_t row0, int64_t nrows, int64_t N, const int32_t* slice_ptr,
                           const int32_t* row_len, const int32_t* s_col, const double* val, const double* diag,
                           int64_t G, const double* u, double* partials, unsigned* ticket, double* red_out,
                           const double* field_rows) {
  hipLaunchKernelGGL(k_reaction<GripField>, MFEA_GRID(grid_rows(nrows > 0 ? nrows : 1)), row0, nrows, N, slice_ptr,
                     row_len, s_col, val, diag, G, u, partials, ticket, red_out, GripField{field_rows},
                     (double*)nullptr);
}

void launch_load_work(hipStream_t s, int64_t nf, const NodeLoad& load, double dy_top, const double* u,
                      double* partials, unsigned* ticket, double* red_out) {
  hipLaunchKernelGGL(k_load_work, MFEA_GRID(grid_rows(nf > 0 ? nf : 1)), nf, load, dy_top, u, partials, ticket,
                     red_out);
}

void launch_stress(hipStream_t s, int64_t E, const int32_t* e2n, const double* xyz,
                   const double* u, Material m, double max_strain, uint8_t* active,
                   double* stress, double* partials, unsigned* ticket, double* red_out,
                   const uint8_t* owned, int32_t* fail_list, unsigned* fail_cnt, const double* Ee,
                   const double* strength) {
  if (Ee || strength)
    hipLaunchKernelGGL(k_stress<ElemPost>, MFEA_GRID(grid_rows(E > 0 ? E : 1)), E, e2n, xyz, u,
                       (ElemPost{m.E, Ee, strength}), max_strain, active, stress, partials, ticket, red_out, owned,
                       fail_list, fail_cnt);
  else
    hipLaunchKernelGGL(k_stress<Material>, MFEA_GRID(grid_rows(E > 0 ? E : 1)), E, e2n, xyz, u, m, max_strain,
                       active, stress, partials, ticket, red_out, owned, fail_list, fail_cnt);
}

int64_t energy_partials(int64_t n_elems) { return 2 * (grid_rows(n_elems > 0 ? n_elems : 1) + kShards); }

void launch_energy(hipStream_t s, int64_t E, const int32_t* e2n, const double* xyz, const double* u,
                   const uint8_t* active, Material m, const double2* sec, const EnergyOut& out, double* partials,
                   unsigned* ticket, double* red_out) {
  if (sec)
    hipLaunchKernelGGL(k_energy<ElemSection>, MFEA_GRID(grid_rows(E > 0 ? E : 1)), E, e2n, xyz, u, active,
                       ElemSection{sec}, out, partials, ticket, red_out);
  else
    hipLaunchKernelGGL(k_energy<Material>, MFEA_GRID(grid_rows(E > 0 ? E : 1)), E, e2n, xyz, u, active, m, out,
                       partials, ticket, red_out);
}

void launch_unfail(hipStream_t s, const int32_t* fail_list, unsigned* cnt, uint8_t* active) {
  hipLaunchKernelGGL(k_unfail, dim3(1), dim3(kBlock), 0, s, fail_list, cnt, active);
}

void launch_floating(hipStream_t s, int64_t n_rows, int64_t n_free, int64_t grip_end, const int32_t* slice_ptr,
                     const int32_t* row_len, const int32_t* s_col, const int32_t* s_elem, const uint8_t* active,
                     int32_t* parent, uint8_t* anchored, const int32_t* label, uint8_t* mask, int tile_rows) {
  if (n_free <= 0) return;
  tile_rows = tile_rows == 512 || tile_rows == 1024 || tile_rows == 4096 ? tile_rows : 2048;
  const int64_t tiles = (n_rows + tile_rows - 1) / tile_rows;
  auto local = tile_rows == 512 ? k_cc_local<512> : tile_rows == 1024 ? k_cc_local<1024>
               : tile_rows == 4096 ? k_cc_local<4096> : k_cc_local<2048>;
  hipLaunchKernelGGL(local, MFEA_GRID(tiles), n_rows, slice_ptr, row_len, s_col, s_elem, active, parent, anchored);
  hipLaunchKernelGGL(k_cc_cross, MFEA_GRID(grid_rows(n_rows)), n_rows, slice_ptr, row_len, s_col, s_elem, active,
                     parent, tile_rows);
  hipLaunchKernelGGL(k_cc_flatten, MFEA_GRID(grid_rows(n_rows)), n_rows, parent, n_free, grip_end, anchored);
  hipLaunchKernelGGL(k_cc_mask, MFEA_GRID(grid_rows(n_free)), n_free, parent, anchored, label, mask);
}

void launch_element_stiffness(hipStream_t s, int64_t n, const double* p1, const double* p2,
                              Material m, double* Ke, double* L) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_element_stiffness, MFEA_GRID(grid_rows(n)), n, p1, p2, m, Ke, L);
}

void launch_csr_rhs_init(hipStream_t s, int64_t n, const int64_t* indptr, const int32_t* indices,
                         const double* data, const uint8_t* known, const double* kval, double reg,
                         double* x, double* r, double* p, double* dinv, double* partials,
                         unsigned* ticket, double* red_out) {
  hipLaunchKernelGGL(k_csr_rhs_init, MFEA_GRID(grid_rows(n > 0 ? n : 1)), n, indptr, indices, data,
                     known, kval, reg, x, r, p, dinv, partials, ticket, red_out);
}

void launch_spmv_csr(hipStream_t s, int j, int64_t n, const int64_t* indptr,
                     const int32_t* indices, const double* data, const uint8_t* known,
                     double reg, const double* p, double* q, Slot* slots, const SolveState* st,
                     double* partials, unsigned* ticket) {
  hipLaunchKernelGGL(k_spmv_csr, MFEA_GRID(grid_rows(n > 0 ? n : 1)), j, n, indptr, indices, data,
                     known, reg, p, q, slots, st, partials, ticket);
}

}  // namespace mfea
