/*
 * mfea.h — C ABI of the MI355X-native mycelium FEA engine (libmfea.so).
 *
 * The reference has no FFI: its hot path is Python calling NumPy/SciPy
 * (src/fea_solver.py) or a C++ main() calling PETSc (src/fea_petsc.cpp).
 * Each entry point below replaces one piece of that path; the reference
 * interface it stands in for is cited beside it.  Plain pointers and sizes
 * only (no torch types).  All functions return 0 on success and a negative
 * MFEA_E* code on failure; mfea_last_error() returns the message of the most
 * recent failure on the calling thread.
 *
 * Ownership: host arrays passed in are caller-owned and copied (or written)
 * synchronously before the call returns.  Device buffers belong to the handle.
 * Threading: one host thread per handle; a handle is not re-entrant.
 * Node/element indices are 0-based rows of nodes.csv / elements.csv
 * (src/fea_petsc.cpp:39-40 — node index = row order).
 */
#ifndef MFEA_H
#define MFEA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 8: MFEA_PC_SOR / MFEA_PC_ICC factorise the whole matrix (were block Jacobi
 *    over 256-row blocks); every preconditioner honours mfea_solve_opts.norm */
#define MFEA_ABI_VERSION 8

/* error / status codes */
#define MFEA_OK 0
#define MFEA_EINVAL -1      /* bad argument (e.g. node id out of range)                */
#define MFEA_EDEVICE -2     /* HIP runtime error                                       */
#define MFEA_ESTATE -3      /* call out of order (no mesh, no BCs, ...)                */
#define MFEA_EMAXIT -4      /* PCG hit max_it (PETSc KSP_DIVERGED_ITS)                  */
#define MFEA_EBREAKDOWN -5  /* PCG breakdown: p·Ap <= 0 or non-finite (KSP_DIVERGED_*) */
#define MFEA_ENOMEM -6
#define MFEA_ECOMM -7       /* RCCL failure (multi-GPU)                                */

/* mesh flags (mfea_set_mesh) */
#define MFEA_MESH_SKIP_INVALID 1u /* skip elements with out-of-range node ids, as
                                     src/fea_petsc.cpp:241 does; default: reject,
                                     as src/fea_solver.py:82-83 would (IndexError) */

/* solver selection (mfea_solve_opts.precond) */
#define MFEA_PC_JACOBI 0        /* PCJACOBI — diagonal of K_ff + reg·I              */
#define MFEA_PC_BLOCK_JACOBI 1  /* 3×3 node-block Jacobi (exact inverse per block)   */
#define MFEA_PC_GAMG 2          /* smoothed-aggregation AMG V-cycle, the counterpart of
                                   the reference sweep's `-pc_type gamg`
                                   (src/fea_petsc_solverAndPC.cpp:330-391).  Partitioned
                                   handles: ONE global hierarchy whose large levels are
                                   split over the ranks (the one-partition iteration
                                   count) or block Jacobi over per-partition ones — per
                                   active set the faster of the two, measured
                                   (mfea_debug.h option "amg_dist") */

#define MFEA_PC_SOR 3           /* `-pc_type sor`: SSOR (ω = 1, PETSc's default) on the
                                   node blocks of the WHOLE K_ff + reg·I, every coupling
                                   kept, factorised in a chain-piece multicolour order
                                   (hyphal chains of ≤ 64 rows keep their natural order;
                                   the pieces of one colour are independent and each
                                   piece's recurrence is a scan across a wave's lanes;
                                   csrc/sweep.hip); one partition */
#define MFEA_PC_ICC 4           /* `-pc_type icc` (the reference source's default PCICC,
                                   src/fea_petsc.cpp:331; also `ilu`, the same factor on
                                   an SPD matrix): DIC(0) — incomplete block Cholesky of
                                   the whole K_ff + reg·I with A's off-diagonal blocks and
                                   f64 pivots D̃_i = D_i − Σ_{j<i} A_ij D̃_j⁻¹ A_ijᵀ — in
                                   the same chain-piece multicolour order as MFEA_PC_SOR */

/* Every preconditioner stops on the norm mfea_solve_opts.norm selects.
 * One-partition MFEA_PC_GAMG solves on MFEA_NORM_UNPRECONDITIONED test ‖r‖₂
 * of a batch's last update directly: n iterations cost n V-cycles, where
 * MFEA_NORM_PRECONDITIONED (its test needs M⁻¹r) costs n + 1; the results
 * have the same bits (option "amg_close", read-only "amg_last_cycles" and
 * "amg_close_hits": mfea_debug.h). */
/* stopping norm (mfea_solve_opts.norm) */
#define MFEA_NORM_UNPRECONDITIONED 0 /* ‖r‖₂ ≤ rtol·‖b‖₂  (SciPy cg; the metric)      */
#define MFEA_NORM_PRECONDITIONED 1   /* ‖z‖₂ ≤ rtol·‖M⁻¹b‖₂ (PETSc KSPCG default)     */

typedef struct mfea_handle mfea_handle;

typedef struct {
  double rtol;      /* relative tolerance; PETSc default 1e-5, metric 1e-8, parity 1e-13 */
  double atol;      /* absolute tolerance on the chosen norm (PETSc default 1e-50)       */
  int32_t max_it;   /* PETSc default 10000                                              */
  int32_t precond;  /* MFEA_PC_*                                                         */
  int32_t norm;     /* MFEA_NORM_*                                                       */
  int32_t chunk;    /* iterations per captured hipGraph replay (0 = library default)     */
  double reg;       /* diagonal regularisation of K_ff, src/fea_solver.py:125 (1e-12)    */
} mfea_solve_opts;

typedef struct {
  int32_t iters;     /* PCG iterations executed                                        */
  int32_t status;    /* 0 converged, MFEA_EMAXIT, MFEA_EBREAKDOWN                       */
  double relres;     /* final ‖r‖/‖b‖ (recursive residual)                               */
  double bnorm;      /* ‖b_f‖₂                                                          */
  int64_t n_free;    /* free DOFs                                                       */
  double t_assemble_ms, t_rhs_ms, t_solve_ms, t_post_ms; /* device time (HIP events),
                        recorded only with option "phase_times" 1 (0 otherwise): an
                        event between two kernels idles the GPU for several µs      */
  double t_setup_ms; /* MFEA_PC_GAMG: numeric hierarchy setup (inside t_solve_ms)     */
  int32_t amg_levels; /* MFEA_PC_GAMG: levels of the hierarchy (0 otherwise)         */
  int32_t amg_rebuilt; /* 1 if this solve rebuilt the symbolic hierarchy (new active set) */
} mfea_stats;

/* ---- lifecycle ------------------------------------------------------------ */
int mfea_abi_version(void);
int mfea_last_error(char* buf, size_t n);
/* One handle drives one device.  Multi-GPU = one process (one handle) per GPU,
 * joined by mfea_dist_init. */
int mfea_create(int device, mfea_handle** out);
int mfea_destroy(mfea_handle* h);

/* Material constants, src/fea_solver.py:14-20 / src/fea_petsc.cpp:23-27. */
int mfea_set_material(mfea_handle* h, double E, double A, double I);

/* ---- per-element section, modulus and failure strain ----------------------- */
/* A heterogeneous network: each column is an array of n_elems doubles indexed
 * by the element's row in the mesh (elements.csv), or NULL for the handle's
 * scalar (E, A, I of mfea_set_material) / the call's scalar (max_strain of
 * mfea_post, mfea_step, mfea_run, mfea_event_opts).  The library copies the
 * arrays.  NULL, or every column NULL: back to the uniform engine.
 *   assembly  k_ax = (E_e·A_e)/L_safe, k_b = ((12·E_e)·I_e)/L_safe³ — the host
 *             forms EA_e = E_e*A_e and EI12_e = (12.0*E_e)*I_e with the
 *             expressions and rounding of mfea_set_material;
 *   post      stress_e = E_e·ε_e; element e fails when |ε_e| > max_strain_e
 *             (+inf: never);
 *   events    see mfea_event.
 * Call order: after mfea_set_mesh (MFEA_ESTATE before it).  mfea_set_mesh
 * clears the properties; mfea_set_bc, mfea_set_active and mfea_set_material
 * keep them — a later mfea_set_material changes only the columns given as NULL.
 * MFEA_EINVAL, the handle unchanged, unless every E, A, I is finite and >= 0
 * and every max_strain is > 0 and not NaN (+inf allowed).
 * One partition only: MFEA_ESTATE on a partitioned handle (mfea_debug_set_parts,
 * an RCCL world); a handle with properties that is partitioned afterwards
 * returns MFEA_ESTATE from its next build.
 * A change drops everything option "keep_operator" keeps (K, the GAMG
 * hierarchy's values) and every captured graph that holds the old properties;
 * the symbolic hierarchy stays (amg_rebuilt == 0): the active set did not move.
 * With "amg_theta_ppm" > 0 the strength estimate weighs each coupling by its
 * element's own EA_e and EI12_e/EA_e.
 * The uniform identity: arrays filled with the handle's scalars and the call's
 * max_strain give K, U, iteration counts, force, stress, activity and n_active
 * bit for bit those of the uniform engine, for every preconditioner (θ = 0).
 * mfea_element_stiffness stays uniform. */
typedef struct {
  const double* E;          /* n_elems, or NULL: the handle's E (mfea_set_material)            */
  const double* A;          /* n_elems, or NULL: the handle's A                                */
  const double* I;          /* n_elems, or NULL: the handle's I                                */
  const double* max_strain; /* n_elems, or NULL: the call's scalar; > 0, +inf = never fails    */
} mfea_element_props;
int mfea_set_element_props(mfea_handle* h, const mfea_element_props* p);
/* What the engine uses, n_elems doubles per non-NULL argument: a column that
 * was not set comes back filled with the handle's scalar — max_strain with
 * NaN, because that scalar belongs to the call, not to the handle. */
int mfea_get_element_props(mfea_handle* h, double* E, double* A, double* I, double* max_strain);

/* ---- grip motion: shear, mixed-mode and out-of-plane tests ------------------ */
/* Direction of the grip motion.  Prescribed displacement of a top-band node =
 * dy_top·top[c], of a bottom-band node = dy_bot·bot[c], c = x, y, z: one f64
 * multiplication per component; dy_top / dy_bot are the amplitudes every
 * solve / step / run / event call already takes.  Default (0,1,0), (0,1,0):
 * the tensile test.  NULL for either = leave it as it is.  Not normalised.
 *   RHS       a free row with a known neighbour of class top or bottom takes
 *             b −= V·p with V the neighbour's whole symmetric 3×3 block and
 *             p[c] = fl(amplitude·direction[c]); each row of V·p is one fma
 *             chain in component order (x, y, z), the neighbours in slot order.
 *             A known row gets x = p.  A node in both bands takes the bottom
 *             value, as in the tensile test.
 *   force     wherever the API returns a force (total_force of mfea_post /
 *             mfea_step, mfea_run_records.force, force1 of events) it is the
 *             work-conjugate one,
 *               F = (top[0]·S[0] + top[1]·S[1]) + top[2]·S[2],
 *               S[c] = Σ_{top rows} (K·U)[3n+c]  (mfea_get_reaction's top),
 *             f64 products and sums in exactly this order, no fused operation.
 *             For (0,1,0) that is the tensile test's F_y.
 *   events    U ∝ amplitude on a fixed active set whatever the direction:
 *             mfea_event's rules stand unchanged, force1 as above.
 * MFEA_EINVAL, the handle unchanged, unless every component given is finite
 * and no vector given is all zero.  The directions are handle state, as the
 * material is: mfea_set_mesh, mfea_set_bc, mfea_set_active, mfea_set_material
 * and mfea_set_element_props keep them.
 * One partition only: MFEA_ESTATE on a partitioned handle; a handle with
 * another direction than the default that is partitioned afterwards returns
 * MFEA_ESTATE from its next build.
 * Default state: at (0,1,0), (0,1,0) — never set, or set explicitly — the
 * handle takes the kernels, launches and graphs of the tensile engine, and
 * every result is bit for bit that engine's, for every preconditioner.
 * A change keeps K, the symbolic hierarchy and everything option
 * "keep_operator" keeps (none depends on the direction: the next step is a
 * kept step, amg_rebuilt == 0); it drops the right-hand side a step cached
 * and every captured graph, which hold the old vectors by value.
 * Planar meshes (every z == 0): with every z component zero the 2-DOF lane
 * path runs as in the tensile test (x and y are both in the plane).  With a
 * non-zero z component in either vector the handle solves with 3 DOFs per
 * node, as option "lane_dof" 3 makes it, and the change takes the rebuild a
 * layout option takes (the activity is kept).  The axial strain of an
 * out-of-plane motion on a planar mesh is zero to first order: no element
 * fails, and an event there is the unloaded terminal event (lam = +inf,
 * MFEA_EVENTS_UNLOADED). */
int mfea_set_grip_motion(mfea_handle* h, const double top[3], const double bot[3]);
int mfea_get_grip_motion(mfea_handle* h, double top[3], double bot[3]);
/* Σ over the band's rows of (K·U)[3n+c], c = x, y, z, on the unregularised K
 * of the last assembly and the current U (MFEA_ESTATE: no assembly since the
 * last build; one partition only).  Either may be NULL.  A node in both bands
 * counts in the bottom one.  The y sum of the top band has total_force's bits
 * in the tensile test. */
int mfea_get_reaction(mfea_handle* h, double top[3], double bot[3]);

/* ---- grip displacement field: a prescribed vector per grip node -------------- */
/* field: 3·n_nodes doubles, original node order, row n = the vector d_n of node
 * n; NULL: no field (back to mfea_set_grip_motion's two vectors).  Copied.
 * Grip rotation d_n = a × (x_n − c), an affine boundary displacement
 * d_n = H·x_n, an indentation (zero rows: held nodes) are fields.
 *   value     with a field, a node n in a band is prescribed
 *             p[c] = fl(a_n·d_n[c]), one f64 product per component, with
 *             a_n = dy_bot if n is in the bottom band, otherwise dy_top (a node
 *             in both bands is a bottom node, as in the tensile test).  Rows of
 *             nodes in no band are stored and otherwise ignored.  While a field
 *             is set the two vectors of mfea_set_grip_motion are read nowhere;
 *             they are kept, still settable and gettable, and take over again
 *             when the field is cleared.
 *   RHS       mfea_set_grip_motion's rule with p per neighbour: a free row with
 *             a known neighbour j takes b −= V·p_j, each row of V·p_j one fma
 *             chain in component order, the neighbours in slot order.  A known
 *             row gets x = p.
 *   force     wherever the API returns a force (total_force, mfea_run_records
 *             .force, force1 of events) it is the generalised force of the top
 *             band, F = Σ_{top rows} w_r,
 *               w_r = (d_r[0]·f_r[0] + d_r[1]·f_r[1]) + d_r[2]·f_r[2],
 *             f_r = (K·U) of row r as mfea_get_reaction accumulates it; f64
 *             products and sums in this order, nothing fused; the rows reduced
 *             in a fixed order, bitwise reproducible for a mesh.
 *             mfea_get_reaction is unchanged: plain component sums.
 *   events    the prescribed displacement stays amplitude × a fixed vector per
 *             node, so U ∝ amplitude on a fixed active set: mfea_event's rules
 *             stand unchanged, force1 as above.
 * MFEA_ESTATE before mfea_set_mesh.  MFEA_EINVAL, the handle unchanged, unless
 * every entry is finite.  Zero rows are legal: a held node.  −0 is stored as 0.
 * Lifetime: mfea_set_mesh clears the field (the node count changes);
 * mfea_set_bc, mfea_set_active, mfea_set_material, mfea_set_element_props and
 * mfea_set_grip_motion keep it; it is gathered into row order again at every
 * build.
 * One partition only: MFEA_ESTATE on a partitioned handle; a handle with a
 * field that is partitioned afterwards returns MFEA_ESTATE from its next build.
 * A change — another field, or NULL — drops exactly what a change of the grip
 * directions drops: the right-hand side a step cached and every captured graph,
 * after draining the stream.  K, the symbolic hierarchy and everything option
 * "keep_operator" keeps stay: the next step is a kept step (amg_rebuilt == 0).
 * Setting the same bytes again drops nothing.
 * Planar meshes (every z == 0): with any z entry of the stored field non-zero
 * the handle solves with 3 DOFs per node, and the change takes the rebuild a
 * layout option takes (the activity is kept); clearing the field, or setting
 * one with every z entry zero, goes back to 2.
 * Uniform identity: a field whose rows equal the band vectors (the top vector
 * on nodes only in the top band, the bottom vector on bottom-band nodes) gives
 * U, iteration counts, stress, activity, n_active, lam and n_failed bit for bit
 * those of mfea_set_grip_motion with these vectors, for every preconditioner;
 * the force differs by summation order only, Σ d·f against d·Σ f. */
int mfea_set_grip_field(mfea_handle* h, const double* field);
/* field (3·n_nodes, may be NULL) as stored; *is_set 0/1 (may be NULL).  Not set:
 * every row filled with the vector its node's band would use (bottom wins),
 * rows of nodes in no band with zeros. */
int mfea_get_grip_field(mfea_handle* h, double* field, int32_t* is_set);
/* The work-conjugate (generalised) force of each band on the unregularised K of
 * the last assembly and the current U; either may be NULL.  States as
 * mfea_get_reaction.  With a field: G = Σ_{band rows} w_r as above; the top
 * value has the bits of the total_force a post of this U returns.  Without:
 *   G = (v[0]·S[0] + v[1]·S[1]) + v[2]·S[2]
 * with v the band's direction and S its sums of mfea_get_reaction; for the top
 * band those are total_force's bits. */
int mfea_get_grip_work(mfea_handle* h, double* top, double* bot);

/* ---- nodal loads: a force vector per free node, dead or proportional --------- */
/* loads: 3·n_nodes doubles, original node order, row n = the force f_n on node
 * n; NULL: no loads (the engine as it is without them; mode is then ignored).
 * Copied.  Self-weight, a point or indenter force, a pre-load under a ramp, a
 * force-controlled pull (a band held by zero rows of a grip field) are loads.
 *   mode      MFEA_LOAD_DEAD: q_n = f_n whatever the amplitudes of the call;
 *             MFEA_LOAD_PROPORTIONAL: q_n[c] = fl(dy_top · f_n[c]), one f64
 *             product per component: f is the load per unit of the top amplitude.
 *   storage   rows of grip nodes are stored and read nowhere (a prescribed DOF
 *             has no load).  −0 is stored as 0, and a product −0 counts as 0.
 *             An all-zero array counts as set: it takes the load kernels, and U,
 *             iteration counts, stress, activity, n_active and force are bit for
 *             bit those of a handle without loads.
 *   RHS       a free row of node n takes b[c] = q[c] − k[c], k the grip term
 *             accumulated as without loads (the fma chains of the tensile test,
 *             mfea_set_grip_motion or mfea_set_grip_field, in slot order), the
 *             subtraction one operation in place of 0 − k[c].  Known rows are
 *             unchanged.  mfea_stats.bnorm and the stopping threshold are those
 *             of this b: a dead load at dy_top = dy_bot = 0 is a real solve.
 *   floating  a free row whose connected component of the active element graph
 *             holds no grip row (a node with no active element included) has its
 *             load dropped, q = 0: it stays at exactly zero for every
 *             preconditioner and entry point, where the regularised system would
 *             return displacements near 1e12.  The mask is that of the activity
 *             the step's K is assembled from — the activity before that step's
 *             failures — recomputed on the device, on the handle's stream,
 *             whenever that activity has moved, and only while loads are set.
 *   force     total_force, mfea_run_records.force, force1, mfea_get_reaction and
 *             mfea_get_grip_work stay as defined: sums over grip rows of K·U.
 *   events    proportional loads scale with the amplitude pair like every other
 *             prescribed quantity, so U ∝ amplitude on a fixed active set and
 *             mfea_event / mfea_run_events stand unchanged.  With dead loads the
 *             response is affine in the load factor: both return MFEA_ESTATE.
 *             mfea_solve, mfea_step and mfea_run work in both modes.
 * MFEA_ESTATE before mfea_set_mesh.  MFEA_EINVAL, the handle unchanged, for an
 * entry that is not finite or an unknown mode.
 * Lifetime: mfea_set_mesh clears the loads (the node count changes);
 * mfea_set_bc, mfea_set_active, mfea_set_material, mfea_set_element_props,
 * mfea_set_grip_motion and mfea_set_grip_field keep them; they are gathered
 * into row order again at every build.
 * One partition only: MFEA_ESTATE on a partitioned handle; a handle with loads
 * that is partitioned afterwards returns MFEA_ESTATE from its next build.
 * A change — other bytes, another mode, or NULL — drops exactly what a change of
 * the grip directions drops: the right-hand side a step cached and every
 * captured graph, after draining the stream.  K, the symbolic hierarchy and
 * everything option "keep_operator" keeps stay: the next step is a kept step
 * (amg_rebuilt == 0).  Setting the same bytes and mode again drops nothing.
 * Planar meshes (every z == 0): with any stored z entry non-zero the handle
 * solves with 3 DOFs per node, by the rule and the rebuild of
 * mfea_set_grip_field; clearing the loads, or setting ones with every z entry
 * zero, goes back to 2. */
#define MFEA_LOAD_DEAD 0
#define MFEA_LOAD_PROPORTIONAL 1
int mfea_set_node_loads(mfea_handle* h, const double* loads /* 3·n_nodes or NULL */, int32_t mode);
/* loads (3·n_nodes, may be NULL) as stored, zeros when not set; *mode and
 * *is_set (0/1) may be NULL. */
int mfea_get_node_loads(mfea_handle* h, double* loads /* may be NULL */, int32_t* mode, int32_t* is_set);
/* The work of the loads, L = Σ q_n·u_n over the free nodes that are not
 * floating, each term (q[0]·u[0] + q[1]·u[1]) + q[2]·u[2] in f64 with nothing
 * fused, the rows reduced in a fixed order (bitwise reproducible for a mesh).
 * The amplitudes and the mask are those of the last solve, U the current one.
 * States as mfea_get_reaction; 0.0 when no loads are set.
 * Work identity with loads (f: the free DOFs, r = b − (K + reg·I)u_f the
 * solver's residual): at equilibrium
 *   u_fᵀ(KU)_f = L − reg·‖u_f‖² − u_f·r
 * so, with G the two values of mfea_get_grip_work,
 *   2W = dy_top·G_top + dy_bot·G_bot + L
 * up to those two terms.  With loads the g rows of mfea_get_energy remain the
 * partial derivatives at fixed U; they are no longer the gradient of the
 * equilibrium energy (the loads' potential −L depends on the parameters through
 * U as well). */
int mfea_get_load_work(mfea_handle* h, double* work);

/* ---- strain energy per element: axial and bending parts, and their gradients - */
/* The element assembled here has two stiffness terms, k_ax = EA_e/L along the
 * filament and k_b = EI12_e/L³ across it (EA_e = E_e·A_e, EI12_e = (12·E_e)·I_e).
 * With δ = u_b − u_a its strain energy ½ δᵀS_eδ is w_axial + w_bending; the
 * axial stress of mfea_get_stress sees the first part only.  One pass over the
 * elements, one lane each; every line one IEEE f64 operation per operator, in
 * this order, nothing fused but inside cube (a = n1, b = n2 of elements.csv):
 *   v_c  = xyz[b][c] − xyz[a][c]
 *   L    = sqrt(vx*vx + vy*vy + vz*vz)          the assembly's expression
 *   Ls   = L < 1e-12 ? 1e-12 : L
 *   n_c  = v_c / Ls
 *   δ_c  = U[b][c] − U[a][c]
 *   d    = (n0*δ0 + n1*δ1) + n2*δ2              axial stretch
 *   t_c  = δ_c − d*n_c                          transverse part
 *   q    = (t0*t0 + t1*t1) + t2*t2
 *   g_axial   = ((0.5*d)*d) / Ls                energy per unit EA_e
 *   g_bending = (0.5*q) / cube(Ls)              energy per unit EI12_e; cube: the
 *                                               assembly's double-double Ls³
 *   w_axial   = EA_e * g_axial      w_bending = EI12_e * g_bending
 * so w = section · g holds exactly, in bits.  An element that does not count
 * (inactive in the mask used, or an endpoint dropped under
 * MFEA_MESH_SKIP_INVALID) gives four zeros.  A zero-length element has n = 0,
 * d = 0, t = δ and w_bending = ½ k_b |δ|², what K holds for it: the result is
 * finite wherever K is (no NaN, unlike that element's strain).
 *   U       3·n_nodes in original node order, or NULL: the handle's current
 *           displacement, what mfea_get_displacement returns;
 *   active  n_elems bytes (nonzero = counts), or NULL: the handle's current
 *           activity.  After a step whose post failed elements, the elements in
 *           that step's K are those of the activity BEFORE it: a caller who
 *           wants the step's equilibrium energy passes that mask;
 *   total   (Σ w_axial, Σ w_bending) over the elements, summed in a fixed order
 *           (bitwise reproducible for a mesh), or NULL;
 *   out     the rows wanted, each n_elems doubles in original element order or
 *           NULL; out itself may be NULL.
 * Gradients.  W = ½ UᵀKU = Σ_e (w_axial + w_bending).  With the grips'
 * displacements prescribed, equilibrium of the free rows makes the implicit
 * term vanish, ∂W/∂θ_e = ½ u_eᵀ(∂K_e/∂θ_e)u_e, so without an adjoint solve
 *   ∂W/∂E_e = A_e·g_axial + (12·I_e)·g_bending
 *   ∂W/∂A_e = E_e·g_axial
 *   ∂W/∂I_e = (12·E_e)·g_bending
 * These are gradients of the equilibrium energy only when U solves the K of
 * `active`; for any other U they are the partial derivatives at fixed U.  When
 * both grips move along the same vector, F = 2W/(dy_top − dy_bot), and the same
 * rows give the gradient of the reported force.
 * Work identity, for any U (S: the sums of mfea_get_reaction, top / bot: the
 * grip directions, f: the free DOFs):
 *   2W = dy_top·(top·S_top) + dy_bot·(bot·S_bot) + u_fᵀ(KU)_f
 * the last term being the solver's residual, zero at equilibrium.  In general,
 * grip field or not, with G the two values of mfea_get_grip_work:
 *   2W = dy_top·G_top + dy_bot·G_bot + u_fᵀ(KU)_f
 * Needs a mesh and boundary conditions, not an assembly (MFEA_ESTATE without
 * them); one partition only (MFEA_ESTATE on a partitioned handle, as
 * mfea_get_reaction).  The call changes nothing a later call can see: no
 * generation moves, nothing option "keep_operator" keeps is dropped (the next
 * step on an unchanged active set is still a kept step), and it is ordered on
 * the handle's stream behind everything enqueued before it, a speculative
 * post's undo included.  A caller's U is permuted to row order on the host and
 * goes into a device buffer allocated at first use. */
typedef struct {
  double* w_axial;   /* n_elems or NULL */
  double* w_bending; /* n_elems or NULL */
  double* g_axial;   /* n_elems or NULL: w_axial per unit EA_e    */
  double* g_bending; /* n_elems or NULL: w_bending per unit EI12_e */
} mfea_element_energy;
int mfea_get_energy(mfea_handle* h, const double* U, const uint8_t* active, double total[2],
                    const mfea_element_energy* out);

/* ---- mesh + boundary conditions (symbolic, once per mesh) ------------------ */
/* Replaces the CSV→array hand-off of fea_solver (src/fea_solver.py:193-201) and
 * read_nodes_csv/read_elems_csv (src/fea_petsc.cpp:42-82, 179-200).
 * xyz: n_nodes×3 row-major f64; e2n: n_elems×2 int64.  Builds the node-block
 * sliced-ELL pattern, the free/known permutation and uploads the mesh. */
int mfea_set_mesh(mfea_handle* h, int64_t n_nodes, const double* xyz, int64_t n_elems,
                  const int64_t* e2n, uint32_t flags);
/* Grip node sets, src/fea_solver.py:207-210 / src/fea_petsc.cpp:203-213.
 * All 3 DOFs of every grip node are prescribed (x=0, y=dy, z=0); a node in
 * both bands takes the bottom value (src/fea_solver.py:226-242 dict order,
 * src/fea_petsc.cpp:292-294 last INSERT wins).  Rebuilds the permutation. */
int mfea_set_bc(mfea_handle* h, int64_t n_top, const int64_t* top, int64_t n_bot,
                const int64_t* bot);
/* Element activity (E bytes, nonzero = active); NULL = all active
 * (src/fea_solver.py:201, src/fea_petsc.cpp:200). */
int mfea_set_active(mfea_handle* h, const uint8_t* active);

/* ---- the hot path ---------------------------------------------------------- */
/* Element stiffness + global assembly on device for the current active set.
 * Replaces bar_stiffness_bulk + assemble_global_stiffness
 * (src/fea_solver.py:30-106) and element_stiffness_6x6 + the MatSetValue loop
 * (src/fea_petsc.cpp:88-140, 229-263). */
int mfea_assemble(mfea_handle* h);
/* Dirichlet elimination, RHS and preconditioned CG on device.
 * Replaces solve_system (src/fea_solver.py:112-135) and MatZeroRowsColumnsIS +
 * diag regularisation + KSPSolve (src/fea_petsc.cpp:286-357).
 * Solves the operator of the last mfea_assemble; a handle (re)built since
 * (mfea_set_mesh / mfea_set_bc, or a layout option of mfea_set_option) is
 * assembled for its current active set first.
 * Returns MFEA_EMAXIT / MFEA_EBREAKDOWN on solver failure (stats still filled);
 * the Python shim maps them to np.linalg.LinAlgError (src/fea_solver.py:250-254). */
int mfea_solve(mfea_handle* h, double dy_top, double dy_bot, const mfea_solve_opts* opts,
               mfea_stats* st);
/* Reaction + stress/failure on device.  Replaces src/fea_solver.py:256-284 and
 * src/fea_petsc.cpp:360-406: total_force = Σ_{top} (K·U)[3n+1] on the
 * unregularised K; stress = E·ε for elements active at step start (0 else);
 * elements with |ε| > max_strain are deactivated for the next step.
 * With per-element properties (mfea_set_element_props): stress_e = E_e·ε_e and
 * element e fails when |ε_e| > max_strain_e; with a strength array the scalar
 * max_strain is otherwise unused (here, in mfea_step and in mfea_run). */
int mfea_post(mfea_handle* h, double max_strain, double* total_force, int64_t* n_active);
/* One full load step = assemble + solve + post (the bench "step").
 * On a handle with one partition the step keeps what the grip displacements
 * do not enter (option "keep_operator", on by default; mfea_debug.h):
 *   - K, while the element activity (mfea_set_active with a mask, failures
 *     reported by a post), the material, the build (mfea_set_mesh / mfea_set_bc,
 *     a layout option) and the assembly kernel are those of the last assembly:
 *     the step then forms only its right-hand side, with the kernel mfea_solve
 *     uses after mfea_assemble;
 *   - the GAMG hierarchy's values, while K, the hierarchy's plan, its floating-
 *     row mask, opts->reg and the smoothing weights are those of the last
 *     numeric setup, and the solve behind that setup converged.
 * rtol, atol and max_it are no inputs of either.  A step that returns an error,
 * any mfea_set_option but "phase_times" / "run_register", a solve with another
 * preconditioner kind (the hierarchy's values only) and the profiling / debug
 * entry points of mfea_debug.h drop what is kept; mfea_assemble always assembles.
 * Results are bit for bit those of a step that assembles and sets up.
 * With "phase_times" a kept step reports the RHS launch as t_assemble_ms and
 * t_setup_ms = 0. */
int mfea_step(mfea_handle* h, double dy_top, double dy_bot, const mfea_solve_opts* opts,
              double max_strain, double* total_force, int64_t* n_active, mfea_stats* st);

/* ---- results (device → host, original node/element order) ----------------- */
int mfea_get_displacement(mfea_handle* h, double* U /* 3·n_nodes, interleaved xyz */);
int mfea_get_stress(mfea_handle* h, double* stress /* n_elems */);
int mfea_get_active(mfea_handle* h, uint8_t* active /* n_elems */);

/* ---- the whole load-step run (one call, records gathered on the device) ----- */
/* The step loop of the drivers (src/fea_solver.py:229-285, src/fea_petsc.cpp:
 * 270-406) as one call: n_steps times mfea_step(h, dy_top[k], dy_bot[k], opts,
 * max_strain, ...) — the same internals, so every option, captured graph and
 * kept-hierarchy rule acts as in a caller's loop — each followed by that
 * step's record rows: what mfea_get_displacement / mfea_get_stress /
 * mfea_get_active would return right after it (U with the grips' prescribed
 * values, stress of the elements active at step start, activity AFTER the
 * step's failures).  A kernel on the handle's stream gathers the rows in
 * original node / element order into one of two device staging slabs; a
 * second stream copies slab k&1 into row k of the caller's arrays while step
 * k+1 computes (the arrays are page-locked with hipHostRegister for the
 * call's duration; where that fails the copies go through two pinned host
 * slabs and a host memcpy — read-only option "run_direct" tells which ran).
 * Starts from the handle's current active set (no mfea_set_active).
 *   - a solver failure at step k (MFEA_EMAXIT / MFEA_EBREAKDOWN) ends the run:
 *     returns 0, *stop_reason = that code, *n_done = k; step k's rows are not
 *     written (the drivers' `break` on LinAlgError, src/fea_solver.py:250-254);
 *   - n_active == 0 after step k ends the run after recording it:
 *     *stop_reason = MFEA_RUN_NO_ACTIVE, *n_done = k + 1 (src/fea_solver.py:283-285);
 *   - any other error is returned as mfea_step returns it (*n_done = the
 *     steps completed and recorded before it).
 * On return every row < *n_done of every non-NULL record is complete in host
 * memory, rows >= *n_done are untouched, and the handle is in the state the
 * last mfea_step left it in (mfea_get_* return the last row).
 * One partition only: a handle with more (mfea_debug_set_parts, an RCCL
 * world) returns MFEA_ESTATE. */
typedef struct {
  double* U;         /* n_steps × 3·n_nodes, row k = step k, original node order; NULL = not kept */
  double* stress;    /* n_steps × n_elems; NULL = not kept                                        */
  uint8_t* active;   /* n_steps × n_elems, activity after the step's failures; NULL = not kept    */
  double* force;     /* n_steps: total_force of step k (required)                                 */
  int64_t* n_active; /* n_steps (required)                                                        */
  mfea_stats* stats; /* n_steps, or NULL                                                          */
  double* wall_s;    /* n_steps, or NULL: host wall time of step k's mfea_step (what the drivers
                        write to solve_runtime.txt)                                               */
} mfea_run_records;

#define MFEA_RUN_COMPLETE 0  /* all n_steps ran                          */
#define MFEA_RUN_NO_ACTIVE 1 /* n_active reached 0 after step n_done - 1 */

int mfea_run(mfea_handle* h, int32_t n_steps, const double* dy_top, const double* dy_bot,
             const mfea_solve_opts* opts, double max_strain, const mfea_run_records* rec,
             int32_t* n_done, int32_t* stop_reason);

/* ---- event-driven failure runs (each break at its exact critical load) ------ */
/* The reference finds failures on a ramp of fixed displacement steps
 * (src/fea_solver.py:216-285): at each step every element over max_strain is
 * failed in one go, so the failure loads depend on the step count, elements
 * that would break one after another go as a batch, and the first break is
 * reported up to one step late.  Between failures the problem is linear in the
 * grip displacement (U ∝ dy on a fixed active set), so ONE solve at a reference
 * load (dy_top, dy_bot) gives the load factor of the next break exactly.  One
 * event — mfea_event — is a mfea_step at the reference load whose post is:
 *   U₁     the solution; F₁ = Σ_top (K·U₁)_y with mfea_post's bits; ε_e the
 *          strain of every active element, mfea_post's expression;
 *   smax   max |ε_e| over the active elements (NaN strains — zero-length
 *          elements — are skipped and never fail);
 *   lam    max_strain / smax, one f64 division (+inf when smax == 0: nothing
 *          is active or the sample has separated — the network is unloaded);
 *   if lam <= lam_max and the network is loaded, every active element with
 *          |ε_e| >= smax·(1 − tie_rtol) fails (product and difference rounded
 *          once each): elements tied up to solver rounding break together.
 *          Otherwise nothing fails: the event is terminal (n_failed == 0);
 *   stress (E·ε_e)·lam for the elements active at event start, 0 otherwise —
 *          the state AT the failure load; on a terminal event the factor is
 *          lam_max when that is finite, else 1.
 * The caller forms force = lam·force1 and displacement = lam·(dy_top − dy_bot).
 * After an event mfea_get_displacement returns U₁ (unscaled), mfea_get_stress
 * the event's stress row, mfea_get_active the activity after its failures.
 * With no active element the event is the unloaded terminal one without a
 * solve: lam = +inf, force1 = 0 (U₁ stays what the last solve left).
 * "keep_operator" keeps nothing from one breaking event to the next — each
 * changes the active set — but the symbolic hierarchy is kept as for steps.
 * MFEA_EINVAL unless max_strain > 0, 0 <= tie_rtol < 1, lam_max > 0 (+inf
 * allowed); one partition only (MFEA_ESTATE otherwise, as mfea_run).
 * With a per-element strength (mfea_set_element_props, max_strain), each of the
 * following one IEEE operation:
 *   lam_e  max_strain_e / |ε_e| over the active, valid elements with |ε_e| > 0
 *          (NaN strains skipped as above);
 *   lam    min_e lam_e, +inf when there is none or every such strength is +inf
 *          (the unloaded terminal event, MFEA_EVENTS_UNLOADED in a run);
 *   if lam <= lam_max (and lam < +inf), every such element with
 *          lam_e <= lam / (1 − tie_rtol) fails (difference and quotient rounded
 *          once each);
 *   stress (E_e·ε_e)·factor, the factor as above.
 * evopts->max_strain is still validated and otherwise unused.  Without a
 * strength array the smax rule above runs unchanged, with E_e in the stress
 * row when E is per element.  On arrays filled with the scalar, lam is bit for
 * bit the uniform one (a correctly rounded division is monotone:
 * min_e fl(m/|ε_e|) = fl(m/max_e |ε_e|)); the failing group can differ from
 * |ε_e| >= smax·(1 − tie_rtol) only for an element within rounding of that
 * boundary. */
typedef struct {
  double max_strain; /* failure strain, src/fea_solver.py:20 MAX_STRAIN                      */
  double tie_rtol;   /* relative width of the failing group below smax (1e-9 is a good default) */
  double lam_max;    /* largest load factor of the test (+inf: none)                          */
} mfea_event_opts;
typedef struct {
  double lam;       /* load factor of the event                                   */
  double force1;    /* F₁, the reaction at the reference load                      */
  int64_t n_failed; /* elements failed by this event (0: terminal)                */
  int64_t n_active; /* active elements after it                                   */
} mfea_event_out;
int mfea_event(mfea_handle* h, double dy_top, double dy_bot, const mfea_solve_opts* opts,
               const mfea_event_opts* evopts, mfea_event_out* out, mfea_stats* st);

/* n_events × mfea_event with the same internals, each followed by its record
 * rows, gathered and copied out as mfea_run's are (its two device slabs, copy
 * stream and page-locking, with the pinned fallback): U row k = lam_k·U₁ (one
 * multiply per entry, on the device), stress row k, activity after event k.
 *   - a solver failure at event k ends the run: returns 0, *stop_reason = that
 *     code, *n_done = k, row k is not written;
 *   - a terminal event k is recorded in full (n_failed[k] == 0): *n_done = k + 1
 *     and *stop_reason = MFEA_EVENTS_LAMBDA_MAX (lam_k > lam_max) or
 *     MFEA_EVENTS_UNLOADED (smax == 0);
 *   - otherwise MFEA_EVENTS_COMPLETE after n_events events.
 * Rows >= *n_done are untouched.  event_of[e] = the event (counted from this
 * call's start) that failed element e, -1 if it is still active or was
 * inactive at the call's start. */
typedef struct {
  double* U;         /* n_events × 3·n_nodes; NULL = not kept */
  double* stress;    /* n_events × n_elems; NULL = not kept    */
  uint8_t* active;   /* n_events × n_elems; NULL = not kept    */
  double* lam;       /* n_events (required)                    */
  double* force1;    /* n_events (required)                    */
  int64_t* n_failed; /* n_events (required)                    */
  int64_t* n_active; /* n_events (required)                    */
  int32_t* event_of; /* n_elems, or NULL                       */
  mfea_stats* stats; /* n_events, or NULL                      */
  double* wall_s;    /* n_events, or NULL: host wall time of event k */
} mfea_event_records;

#define MFEA_EVENTS_COMPLETE 0   /* all n_events ran, each with failures       */
#define MFEA_EVENTS_LAMBDA_MAX 1 /* event n_done - 1 needs lam > lam_max        */
#define MFEA_EVENTS_UNLOADED 2   /* event n_done - 1 found no strain (smax == 0) */

int mfea_run_events(mfea_handle* h, int32_t n_events, double dy_top, double dy_bot,
                    const mfea_solve_opts* opts, const mfea_event_opts* evopts,
                    const mfea_event_records* rec, int32_t* n_done, int32_t* stop_reason);

/* ---- reference-API helpers ------------------------------------------------- */
/* bar_stiffness_bulk on device (src/fea_solver.py:30-68): Ke n×36 row-major, L n. */
int mfea_element_stiffness(mfea_handle* h, int64_t n, const double* p1s, const double* p2s,
                           double E, double A, double I, double* Ke, double* L);
/* Export the assembled global K (active elements only) as scalar CSR over the
 * 3·n_nodes DOFs in original order, same pattern as the reference's
 * csr_matrix (explicit zeros kept, duplicates summed).  Call with indptr ==
 * NULL to query *nnz. */
int mfea_export_csr(mfea_handle* h, int64_t* nnz, int64_t* indptr, int32_t* indices,
                    double* data);
/* solve_system(K, known_dofs, known_vals) for an arbitrary caller-supplied
 * scalar CSR K (src/fea_solver.py:112-135), on device. U: n out. */
int mfea_solve_csr(mfea_handle* h, int64_t n, const int64_t* indptr, const int32_t* indices,
                   const double* data, int64_t n_known, const int64_t* known_dofs,
                   const double* known_vals, const mfea_solve_opts* opts, double* U,
                   mfea_stats* st);

/* ---- introspection / measurement ------------------------------------------- */
typedef struct {
  int64_t n_nodes, n_elems;
  int64_t n_free_nodes;     /* free rows (3 DOF each)                               */
  int64_t n_top, n_known;   /* grip rows                                            */
  int64_t n_slices;         /* SELL-64 slices                                       */
  int64_t n_slots;          /* slot rows × 64 = allocated slot entries              */
  int64_t free_incidences;  /* Σ row_len over free rows = valid slots the SpMV reads */
  int32_t planar;           /* all z == 0                                           */
  int32_t cg_lanes;         /* 1: CG iterations run on the wave-local lane operator */
  int64_t n_lanes;          /* lanes of that operator (owners + helpers + padding)   */
  int64_t n_halo;           /* lanes with an out-of-wave slot (one push per iteration) */
  int32_t n_parts;          /* partitions of the solve (ranks, or mfea_debug_set_parts)  */
  int32_t part;             /* this handle's (first) partition                         */
  int64_t n_pairs;          /* cut free-free elements of that partition (records/iter)  */
  int64_t n_ghost;          /* its ghost rows (other partitions' nodes)                */
  int32_t halo_compact;     /* lane operator: 1 compact halo records, 0 one per lane   */
  int32_t block_size;       /* lane CG kernels: threads per block                      */
  int64_t grid;             /* lane CG kernels: blocks per launch                      */
} mfea_info;
int mfea_get_info(mfea_handle* h, mfea_info* info);
/* Launches the dominant kernel — the fused SpMV + single-reduction CG iteration —
 * `reps` times on the handle's stream between two HIP events (on the current
 * vectors, identical work each launch) and returns the average launch duration.
 * Call after mfea_solve (it overwrites the solver state). */
int mfea_profile_iteration(mfea_handle* h, int precond, int reps, double* avg_ms);
/* MFEA_PC_GAMG: the SpMV kernel alone — w = A_0 u (f64 blocks) with the CG's
 * four partial sums — replayed `reps` times back to back as one captured
 * graph between two HIP events; average launch duration.  After a GAMG solve
 * (partitioned handles: the first partition's kernel over its own rows). */
int mfea_profile_spmv(mfea_handle* h, int reps, double* avg_ms);

/* ---- record writer (host only: needs no device, no handle) ------------------ */
/* Writes one of the driver's end-of-run CSV records, byte-identical to the
 * reference's writers: src/fea_solver.py:297-316 (pandas to_csv — shortest
 * round-trip floats as numpy/Python repr, NaN as an empty field, True/False,
 * node_displacements headed 0..n_cols-1) with style MFEA_CSV_PANDAS, or
 * src/fea_petsc.cpp:433-516 (setprecision(12), 1/0, node_i_x…node_i_z header)
 * with MFEA_CSV_PETSC.  values: n_rows×n_cols row-major f64 (STRESS, DISP,
 * FORCE); flags: n_rows×n_cols bytes (ACTIVE).  Rows get the 1-based step
 * column, except FORCE (n_cols = 2: total_displacement, total_force).
 * n_threads formats column chunks in parallel (output identical for any). */
#define MFEA_CSV_PANDAS 0
#define MFEA_CSV_PETSC 1
#define MFEA_REC_STRESS 0 /* stress_record.csv       */
#define MFEA_REC_ACTIVE 1 /* active_elements.csv     */
#define MFEA_REC_DISP 2   /* node_displacements.csv  */
#define MFEA_REC_FORCE 3  /* force_displacement.csv  */
int mfea_write_record_csv(const char* path, int style, int kind, int64_t n_rows, int64_t n_cols,
                          const double* values, const uint8_t* flags, int n_threads);
/* The same record as a NumPy .npy sidecar (the CSV's text is what
 * dominates at 1 M DOF; a binary copy reloads in milliseconds): the raw
 * n_rows × n_cols array without the step column, '<f8' (values) or '|b1'
 * (flags, ACTIVE), C order, readable by np.load(allow_pickle=False). */
int mfea_write_record_npy(const char* path, int kind, int64_t n_rows, int64_t n_cols, const double* values,
                          const uint8_t* flags);

/* ---- network producer (host only) ------------------------------------------- */
/* The hyphal growth model of src/mycelium_sim_2D.cpp (main :529-588, process
 * functions :236-414), native and multi-threaded, for networks of millions of
 * nodes.  With mfea_grow_default_params (the reference's
 * constants :17-33, 5×5 inoculum, 150 steps, seed 42) and snapshot_every = 1
 * it writes byte-identical nodes.csv / elements.csv (export_geometry :477-515),
 * mycelium_growth_stats.csv and snapshots/step_NNNN.csv to the reference
 * binary's.  Larger networks: more inoculation sites / a larger dish / more
 * steps (substrate_E and omega0 are totals: scale them with the area). */
typedef struct {
  uint64_t seed;                     /* mt19937_64 seed (:17, argv[1])              */
  double h0, dt, lambda_angle, P_branch, c_g, D, M_cap, omega0;
  int32_t t_steps, h0_per_point;     /* growth steps; hyphae per inoculation site   */
  double anastomosis_tol, wall_thickness, dish_size, substrate_width, substrate_E;
  int32_t inoc_nx, inoc_ny;          /* inoculum grid (:143-159), centred           */
  double inoc_dist;                  /* its spacing, mm                             */
  double voxel_size;                 /* spatial hash voxel (:553, 0.1 mm)           */
  int32_t snapshot_every;            /* 0: none; k: step_%04d.csv every k steps      */
  const char* snapshot_dir;          /* where the snapshots go (must exist)          */
  int32_t verbose;                   /* 1: the reference's stderr progress lines     */
  int32_t threads;                   /* 0: all hardware threads; results identical   */
} mfea_grow_params;
typedef struct mfea_grow_net mfea_grow_net;
void mfea_grow_default_params(mfea_grow_params* p);
int mfea_grow(const mfea_grow_params* p, mfea_grow_net** out);
int mfea_grow_info(const mfea_grow_net* g, int64_t* n_nodes, int64_t* n_elems, int64_t* n_hyphae);
/* xyz (3·n_nodes) as nodes.csv carries them (6 significant digits, read back);
 * e2n (2·n_elems) 0-based node rows as elements.csv.  Either may be NULL. */
int mfea_grow_mesh(const mfea_grow_net* g, double* xyz, int32_t* e2n);
/* nodes.csv, elements.csv and mycelium_growth_stats.csv into dir (must exist) */
int mfea_grow_write(const mfea_grow_net* g, const char* dir);
void mfea_grow_free(mfea_grow_net* g);

/* ---- multi-GPU (one process per GPU, RCCL over xGMI) ----------------------- */
/* Replaces the PETSC_COMM_WORLD row-block distribution of
 * src/fea_petsc_parallel.cpp:169-171, 234-268, 330-409 and its MPI reductions.
 * unique_id: the 128-byte ncclUniqueId made by rank 0 (mfea_dist_unique_id)
 * and broadcast by the caller.  Every rank then passes the WHOLE mesh and the
 * same grips to mfea_set_mesh / mfea_set_bc; the handle keeps the part of the
 * network it owns (partition.hpp: a px × py grid of strips with equal
 * free-node counts, boundaries at the fewest crossing elements), the elements
 * touching it and the far ends of cut elements as ghost rows.
 * Exchanges per CG iteration (one RCCL group of point-to-point transfers each):
 *   Jacobi / block Jacobi — one kernel per GPU, one group (the cut rows' CG
 *     records to the neighbours + the 4 partial sums to every rank);
 *   GAMG (distributed V-cycle) — per split level a halo of the smoother's x
 *     and of the residual on the way down and of the coarse correction and x
 *     on the way up, one all-gather into the first replicated level, the u
 *     halo of w = A u and the sums: 4·(split levels) + 2 groups.
 * All ranks derive bitwise identical α, β and stopping decisions.
 * Partitioned handles: mfea_get_displacement writes the owned nodes' entries,
 * mfea_get_stress / mfea_get_active the entries of elements whose first node
 * is owned (others untouched; mfea_gather_results collects all on rank 0);
 * mfea_post returns the global force and count. */
int mfea_dist_unique_id(uint8_t* unique_id /* 128 bytes */);
int mfea_dist_init(mfea_handle* h, int rank, int world, const uint8_t* unique_id);
/* Partition layout: 0 = strips along x, 1 = along y, -1 (default) = the
 * px × py grid (a factorisation of the world size) whose boundaries cross the
 * fewest elements (partition.hpp).  Takes effect at the next build. */
int mfea_set_partition_axis(mfea_handle* h, int axis);
/* Which nodes / elements this handle reports (1 = its own): every node
 * belongs to one partition, every element to the partition of its first
 * node.  Either array may be NULL.  One partition: all ones. */
int mfea_get_ownership(mfea_handle* h, uint8_t* node_owned /* n_nodes */, uint8_t* elem_owned /* n_elems */);
/* The step's records gathered on rank 0 — the displacement of every node and
 * the stress / activity of every element, as one partition would return them
 * (the reference gathers U to rank 0, src/fea_petsc_parallel.cpp:373-378,
 * while every rank writes the same record files, :491-574; here rank 0 alone
 * writes).  Collective over the RCCL world: every rank calls it; rank 0's
 * arrays are filled, the others' are not touched (may be NULL).  Handles
 * without an RCCL world fill the arrays directly.  Any array may be NULL. */
int mfea_gather_results(mfea_handle* h, double* U /* 3·n_nodes */, double* stress /* n_elems */,
                        uint8_t* active /* n_elems */);

#ifdef __cplusplus
}
#endif
#endif /* MFEA_H */
