/*
 * vaspfsi.h — C-ABI of the MI355X-native monolithic ALE-FSI time-step kernel (libvaspfsi.so).
 *
 * Drop-in boundary.  VaSP's simulation stage hands its problem files to turtleFSI, whose
 * hot loop is, per Newton iteration, `assemble(J_nonlinear)` (+ `A_pre`, `ident_zeros`, `bc.apply(A)`),
 * `assemble(-F)`, `bc.apply(b, u)`, `LUSolver.solve`, `axpy`, `bc.apply(u)` and two norms
 * (turtleFSI/modules/newtonsolver.py `solver_setup` / `newtonsolver`; call sites in the reference:
 * src/vasp/simulations/offset_stenosis.py:9 `from turtleFSI.problems import *`, the hooks at :27,:85,:143,
 * :151,:199,:216 and the solver keys at :44-48).  Each entry point below names the reference-side call it
 * replaces.  All buffers are caller-owned host memory unless stated otherwise; every function returns an
 * `int` status (FSI_OK == 0) and never throws across the ABI.  One host thread per context; contexts are
 * independent (one per GPU).
 *
 * Global dof layout at this boundary ("user layout", vasp_amd/mesh.py): [ d: 3*N2 | v: 3*N2 | p: V ],
 * component-minor, N2 = #P2 nodes (vertices first, then edges), V = #vertices.
 */
#ifndef VASPFSI_H
#define VASPFSI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FSI_OK 0
#define FSI_ERR_INVALID 1      /* bad argument / inconsistent mesh arrays                                   */
#define FSI_ERR_DEVICE 2       /* HIP runtime error (no device, out of memory, launch failure)              */
#define FSI_ERR_DIVERGED 3     /* residual or update > 1e20 or NaN: the reference raises RuntimeError here   */
#define FSI_ERR_LINEAR 4       /* Krylov breakdown / no convergence within max iterations                    */
#define FSI_ERR_PIVOT 5        /* zero or non-finite pivot in the incomplete factorisation                   */

typedef struct FsiCtx FsiCtx;

/* Mesh + discrete-problem description.  Replaces: Mesh/MeshFunction reads and
 * FunctionSpace(mesh, MixedElement([P2^3, P2^3, P1])) in turtleFSI monolithic.py, driven by
 * get_mesh_domain_and_boundaries [REF src/vasp/simulations/offset_stenosis.py:85-140]. */
typedef struct FsiMeshDesc {
  int64_t num_vertices;        /* V                                                                         */
  int64_t num_nodes;           /* N2 = V + #edges                                                           */
  int64_t num_cells;           /* C                                                                         */
  const double* coords;        /* [V][3] vertex coordinates                                                 */
  const int32_t* tet_nodes;    /* [C][10] P2 node ids, UFC local order (4 vertices, 6 edges), rows of the   */
                               /*         vertex part ascending                                             */
  const int32_t* cell_kind;    /* [C] 0 = fluid, 1 = solid.  Cell ORDER is the caller's and is kept (every cell    */
                               /* index of this API refers to it); it decides the locality of the element       */
                               /* kernels: hand the cells over along a space-filling curve (the Python binding   */
                               /* does: vasp_amd.capi.cell_locality_order), not in sweeps over the domain        */
  const int32_t* cell_region;  /* [C] index into fluid_props / solid_props                                  */
} FsiMeshDesc;

/* Material / scheme parameters.  Replaces: fluid_properties / solid_properties lists, dt, theta handed to
 * fluid_setup / solid_setup / extrapolate_setup [REF offset_stenosis.py:36-80; SURVEY.md §8a a4-a6]. */
typedef struct FsiParams {
  double dt;
  double theta;
  int32_t num_fluid_regions;
  const double* fluid_props;   /* [nf][2]  rho_f, mu_f                                                      */
  int32_t num_solid_regions;
  const double* solid_props;   /* [ns][6]  rho_s, mu_s, lambda_s, C10, C01, C11 (the last three: MooneyRivlin)      */
  const int32_t* solid_models; /* [ns]     0 = StVenantKirchoff, 1 = MooneyRivlin                           */
  double delta;                /* d_t = v penalty in the solid (turtleFSI solid.py: 1e7)                    */
  double laplace_alpha;        /* mesh-lifting coefficient ("constant": 1.0)                                */
} FsiParams;

typedef struct FsiNewtonOpts {
  double atol, rtol;           /* newtonsolver(): loop while rel_res > rtol and residual > atol             */
  int32_t max_it;
  double lmbda;                /* relaxation of the update                                                  */
  int32_t recompute;           /* re-assemble the Jacobian every `recompute` Newton iterations              */
  int32_t recompute_tstep;     /* ... and every `recompute_tstep` time steps                                */
  int32_t counter;             /* time-step counter of this call                                            */
  int32_t first_step_num;      /* counter value of the first step of this run (forces a Jacobian)           */
  double lin_rtol;             /* Krylov stop: ||r|| <= eta ||b|| (row-equilibrated norms),                  */
                               /* eta = max(lin_rtol, min(1e-2, f atol / ||b||_newton)), f = 1e-2 unless      */
                               /* fsi_set_newton_forcing changed it (f = 0: eta = lin_rtol, the direct-LU    */
                               /* policy of the reference)                               (inexact Newton)   */
  int32_t lin_max_it;          /* Krylov iteration cap per linear solve                                     */
  int32_t lin_solver;          /* 0 = GCR with recycled directions, 1 = BiCGStab                            */
} FsiNewtonOpts;

typedef struct FsiNewtonIter {
  double residual;             /* ||b||_2   ("r (atol)")                                                    */
  double rel_res;              /* ||du||_L2(Omega), dolfin.norm(Function, 'l2')  ("r (rel)")                */
  int32_t recomputed;          /* 1 if "Compute Jacobian matrix" happened before this iteration             */
  int32_t lin_iters;           /* Krylov iterations (new directions) of this iteration's linear solve       */
  double lin_relres;           /* achieved ||r||/||b||                                                      */
} FsiNewtonIter;

/* ---- tuning ---------------------------------------------------------------------------------------- */
/* Every product option of a context in one place: storage precisions, sizes, Newton / Krylov policy, the preconditioner's
 * structure and sweep counts (DESIGN.md sections 4 - 5 give the measurement behind each default).  fsi_tuning_defaults fills
 * the defaults; fsi_create takes the defaults with the developer overrides of the environment applied (FSI_<NAME> for the
 * field <name>, parsed in ONE function: csrc/fsi_tuning.hip; debugging aids FSI_DEBUG* are not options and stay environment
 * only); fsi_create_tuned takes the struct as given.  The reference has no counterpart: its linear solver is
 * `linear_solver="mumps"` [REF src/vasp/simulations/offset_stenosis.py:45]. */
typedef struct FsiTuning {
  int32_t struct_size;         /* in / out in every call that takes an FsiTuning*: set it to the caller's sizeof(FsiTuning) (0 = this
                                * header's).  fsi_tuning_defaults / _from_env / fsi_get_tuning write at most that many bytes and store
                                * the number written; fsi_create_tuned reads that many and takes the defaults for the rest. */
  /* storage precisions (all arithmetic on the Newton level and every linear-solve verdict is FP64 whatever these say) */
  int32_t krylov_fp32;         /* Krylov basis Q: 0 FP64, 1 FP32, 2 decided per Jacobian lifetime from the tolerances asked for    */
  int32_t operator_fp32;       /* 1: products inside Krylov iterations on an FP32 copy of the Jacobian values (with an FP32 basis) */
  int32_t schur_fp32;          /* 1: Schur-complement sweeps on FP16 / FP32 matrix values (vectors FP64); 0: FP64 values           */
  int32_t sweeps_fp32;         /* 1: velocity / displacement block sweeps in FP32 vectors                                          */
  int32_t sweeps_fp16;         /* 1: fine-level sweep matrices as packed FP16 records                                              */
  int32_t solid_fp32;          /* 1: solid velocity block as FP32 3x3 block-CSR                                                    */
  int32_t pv_fp32;             /* 1: FP32 node-form copies of A_vp / A_pv for the two block products of the pressure step          */
  int32_t krylov_capacity;     /* kept directions per Jacobian lifetime (bounded by half of the free HBM)                          */
  double krylov_fp32_floor;    /* krylov_fp32 == 2: FP32 basis iff the lowest linear tolerance the lifetime can be asked for is    */
                               /* above this.  1e-10 since round 4 (1e-7 before): with the columns kept orthonormal (round 3) the  */
                               /* FP32 basis + restarts from the FP64 residual reach 1e-11 on the golden runs, and the aneurysm    */
                               /* problem at its own tolerances (1e-10 / 1e-9) runs 28 % faster (profiles/r04_aneurysm_fp32.txt)   */
  /* assembly and numbering */
  int32_t assembly_atomic;     /* 0: bitwise reproducible assembly (per-dof gather, cell colours); 1: unordered atomics            */
  int32_t node_order;          /* 0: Morton curve (default), 1: the mesh's order, 2: multicolour (needed by precond = 1)           */
  int32_t tiles;               /* 1: LDS-tiled sweep kernels                                                                        */
  int32_t tile_nodes;          /* nodes per workgroup of the tiled displacement / fluid sweeps: 128 | 256; 0 = 256                     */
  int32_t schur_tile_rows;     /* rows per workgroup of the tiled Schur sweep: 64 | 128 | 256; 0 = 64 (256 in rounds 2-3)               */
  int32_t jacobian_waves;      /* waves per SIMD the refresh kernel's register budget is set for (1 | 2)                           */
  int32_t jacobian_mfma;       /* 1: element contraction of the refresh kernel on v_mfma_f64_16x16x4 (k_jacobian_mfma; measured    */
                               /*    slower in round 4: 103 against 70 ms per refresh at 1.12 M tets)                              */
  /* Newton / Krylov policy */
  double newton_forcing;       /* linear tolerance = forcing * atol / |b| (0: every system to lin_rtol)                            */
  double newton_forcing_late;  /* ... of late Newton iterations (previous update within newton_late_factor of its tolerance)       */
  double newton_late_factor;
  double f32_cycle_floor;      /* FP32 basis: a cycle reduces the residual by at most this factor before the FP64 verdict          */
  double f32_verdict_skip_rtol;/* FP32 basis, inside fsi_newton_solve: answers asked for at or above this may skip the verdict     */
  double orth_floor32, orth_floor64;   /* estimated orthogonality error of a new column that forces a second Gram-Schmidt pass     */
  double gcr_escape;           /* alpha^2 <= this |r|^2: the next direction is made from the last q instead of r                   */
  double gcr_reorth;           /* second Gram-Schmidt pass when |w'| < reorth |w| (0: automatic)                                   */
  /* block preconditioner */
  int32_t prec_streams;        /* 1: two chains of an application side by side on two HIP streams                                  */
  int32_t experiment;          /* measurement switches of the block factorisation, 0 in production: bit 0       */
                               /* pressure right-hand side from the fluid predictor only, bit 1 displacement block without velocity   */
                               /* coupling, bit 2 every Chebyshev chain launches its last sweep (its product is read by nobody; by    */
                               /* default the chain's consumer adds the last direction to x instead: same bits, one launch less)      */
  int32_t cheb4;               /* bit 0 / 1 / 2: 4th-kind Chebyshev sweeps in the solid cycle / displacement cycle / Schur solve   */
                               /* (bit 2 acts on the FP16 / FP32-matrix Schur sweeps only: the all-FP64 fused sweeps ignore it)    */
  int32_t coarse_power;        /* 1: coarse-level Chebyshev intervals from a power iteration (0: Gershgorin bound)                 */
  int32_t solid_mg, dd_mg;     /* two-level (P2 -> P1) cycles of the solid velocity block / the displacement block                 */
  int32_t mg_keep;             /* 1: keep the displacement block's coarse operator while three checksums say it is unchanged       */
  int32_t solid_block_jacobi, solid_fused, fused_sweeps, scalar_dd;
  int32_t its_solid, its_fluid, its_schur, its_disp;          /* sweeps (solid / disp: one-level fallbacks)                         */
  double kappa_solid, kappa_fluid, kappa_schur, kappa_disp;   /* assumed condition numbers of the Chebyshev intervals              */
  int32_t sbmg_pre, sbmg_post, sbmg_cits;                     /* solid cycle: smoothing sweeps before / after, coarse sweeps       */
  double sbmg_alpha, sbmg_ckappa;                             /* ... smoothing interval [lmax / alpha, lmax], coarse kappa         */
  int32_t mg_pre, mg_post, mg_cits;                           /* displacement cycle; mg_post 0 (default) = by context size: 7 below */
                                                              /* 1.1 M P2 nodes, 5 above (fsi_get_tuning returns what was taken)     */
  double mg_alpha, mg_ckappa;
  /* round 5 (fields are appended: struct_size tells an older caller's struct from this one) */
  int32_t solid_coarse_exact;  /* 1: the solid cycle's coarse level is solved exactly - block cyclic reduction over breadth-first levels of
                                * the solid vertices, operators refreshed with the Jacobian (csrc/fsi_bcr.hip) - instead of sbmg_cits sweeps */
  int32_t compact_drows;       /* 1: the outer product takes the three displacement rows of a node from a pair form - [dd_ii, dv_ii] per
                                * node pair, six values instead of 18 + pressure columns - extracted at every Jacobian refresh together
                                * with a check that those rows hold nothing else (they do not for the forms of SURVEY.md A.2: the mesh
                                * extension and the solid's d - v relation act per component); 0: all six value rows are streamed */
  double bcr_shift;            /* ... of A_c + bcr_shift * blockdiag(A_c): the floor below which the level's modes are damped, not inverted */
  double newton_adaptive;      /* linear tolerance >= this x the contraction the Newton iteration of the same index reached one time
                                * step ago under the same Jacobian (net of its own linear tolerance); 0: off.  fsi_newton_solve */
} FsiTuning;
void fsi_tuning_defaults(FsiTuning* t);
/* (internal helper of fsi_get_tuning, exported so that the ABI test can exercise the size rule without a device) */
void fsi_tuning_copy_out(const FsiTuning* full, FsiTuning* out);
/* the defaults with the FSI_<NAME> variables of the environment applied (what fsi_create uses) */
void fsi_tuning_from_env(FsiTuning* t);

/* ---- lifetime ------------------------------------------------------------------------------------ */
/* Replaces: space / form set-up up to solver_setup() (A_pre assembled at the zero state). `device` is the
 * HIP device ordinal. */
int fsi_create(const FsiMeshDesc* mesh, const FsiParams* params, int device, FsiCtx** out);
/* fsi_create with an explicit FsiTuning (the environment is not consulted).  tuning == NULL: the defaults. */
int fsi_create_tuned(const FsiMeshDesc* mesh, const FsiParams* params, int device, const FsiTuning* tuning, FsiCtx** out);
/* the tuning the context was created with */
int fsi_get_tuning(const FsiCtx* ctx, FsiTuning* out);
int fsi_destroy(FsiCtx* ctx);
const char* fsi_last_error(const FsiCtx* ctx);

/* ---- boundary data ------------------------------------------------------------------------------- */
/* Replaces: bcs = [DirichletBC(...), ...] [REF offset_stenosis.py:170-179].  `dofs` are unique user-layout
 * dofs with list-order precedence already resolved. */
int fsi_set_dirichlet(FsiCtx* ctx, int64_t n, const int64_t* dofs);
/* Replaces: per-step expression updates in pre_solve [REF offset_stenosis.py:199-208]; values[i] belongs to dofs[i]. */
int fsi_set_dirichlet_values(FsiCtx* ctx, int64_t n, const double* values);
/* Replaces: F_solid_linear += P * inner(n('+'), psi('+')) * dS(fsi_id) [REF offset_stenosis.py:184-190].
 * `facet_nodes` [nf][6] P2 nodes (3 vertices, 3 edges (b,c),(a,c),(a,b)); `plus_cell` [nf] the '+' cell. */
int fsi_set_pressure_facets(FsiCtx* ctx, int64_t nf, const int32_t* facet_nodes, const int32_t* plus_cell);
/* Replaces: InterfacePressure.update(t) -> P [REF src/vasp/simulations/simulation_common.py:371-395]. */
int fsi_set_interface_pressure(FsiCtx* ctx, double P);
/* Replaces: robin_bc terms of solid_setup [REF src/vasp/simulations/aneurysm.py:73-76]. */
int fsi_set_robin_facets(FsiCtx* ctx, int64_t nf, const int32_t* facet_nodes, const double* k_s, const double* c_s);
/* Inexact Newton: fsi_newton_solve asks the linear solver for max(lin_rtol, min(1e-2, forcing * atol / |b|)).  The
 * reference solves every Newton system with a direct LU (MUMPS); forcing = 0 reproduces that policy (every solve to
 * lin_rtol) for parity runs, the default 1e-2 leaves the Newton iteration counts of the bench unchanged and saves the
 * Krylov iterations that would polish an update far below the Newton tolerance. */
int fsi_set_newton_forcing(FsiCtx* ctx, double forcing);
/* Replaces: `linear_solver="mumps"` [REF offset_stenosis.py:45].  precond 0 = field-split block preconditioner (velocity /
 * pressure SIMPLE split with the solid displacement eliminated, then the displacement block; every inner solve a fixed number
 * of Jacobi-Chebyshev sweeps), 1 = multicolour ILU(0) of the monolithic matrix (needs the context created with
 * FSI_ORDER=colour).  With FsiNewtonOpts.lin_solver (0 recycled GCR, 1 BiCGStab) that makes four pairs; tested on MI355X
 * (tests/test_gpu_parity.py::test_bicgstab_and_ilu0_solve_match_sparse_lu): GCR + field split (the default) and each option
 * with the other's default partner converge to 1e-10; BiCGStab + ILU(0) together stagnates on the FSI Jacobian (a saddle
 * point with 1e7 penalty rows) and is recorded there as a strict xfail. */
int fsi_set_linear_solver(FsiCtx* ctx, int32_t precond);
/* Sweep counts and assumed condition numbers of the Chebyshev solves inside the block preconditioner (solid and
 * fluid-interior part of the velocity block, pressure Schur complement).  Non-positive arguments keep the current value.
 * Defaults (csrc/fsi_tuning.hip is the one place that holds them): solid 300 / 1e4 (one-level fallback; default: the two-level cycle,
 * 16 + 16 sweeps around the exact coarse solve), fluid 4 / 5, Schur 30 / 1e2, displacement 60 / 1e3 (one-level fallback; the default
 * displacement solve is the two-level P2 -> P1 cycle: 3 + 5 smoothing sweeps - 3 + 7 in contexts below 1.1 M nodes - around 16 coarse
 * sweeps). */
int fsi_set_chebyshev(FsiCtx* ctx, int32_t its_solid, double kappa_solid, int32_t its_fluid, double kappa_fluid,
                      int32_t its_schur, double kappa_schur, int32_t its_disp, double kappa_disp);
/* Finishes set-up: assembles A_pre = assemble(J_linear) at the current state (solver_setup()). */
int fsi_solver_setup(FsiCtx* ctx);

/* ---- the hot path --------------------------------------------------------------------------------- */
/* b = assemble(-F); [bc.apply(b, u)]; writes ||b||_2 */
int fsi_assemble_residual(FsiCtx* ctx, double* norm);
/* A = assemble(J_nonlinear) + A_pre; ident_zeros; [bc.apply(A)]; refreshes the preconditioner */
int fsi_assemble_jacobian(FsiCtx* ctx);
/* One linear solve A du = b with the current factorisation (up_sol.solve). */
int fsi_solve(FsiCtx* ctx, double lin_rtol, int32_t lin_max_it, int32_t lin_solver, int32_t* iters, double* relres);
/* newtonsolver(): one time step.  `iters` has room for opts->max_it entries; *n_iters receives the count. */
int fsi_newton_solve(FsiCtx* ctx, const FsiNewtonOpts* opts, FsiNewtonIter* iters, int32_t* n_iters);
/* dvp_["n-1"] <- dvp_["n"] (the reference's vector shift after each step). */
int fsi_shift(FsiCtx* ctx);

/* ---- element partition across GPUs (one context per GPU) --------------------------------- */
/* Replaces: the MPI-parallel dolfin path of `mpirun -np N turtleFSI ...` (ghost updates of PETSc vectors,
 * MPI sums inside the Krylov solver and in norm(); the reference's own MPI use at this boundary:
 * src/vasp/simulations/simulation_common.py:213-220).  The context holds the cells that touch a node it owns
 * (owned cells first in FsiMeshDesc, then the ghost layer); rows of nodes owned elsewhere ("ghost" dofs) are
 * carried as identity rows and are refreshed from their owner once per Krylov iteration.  The library packs
 * `send_dofs` into `sendbuf_dev`, calls `halo_exchange` and unpacks `recvbuf_dev` into `ghost_dofs`; both buffers
 * are device memory owned by the caller (length n_send / n_ghost doubles), the callbacks are the caller's transport
 * (RCCL through torch.distributed in vasp_amd/partition.py).  Callbacks return 0 on success. */
typedef struct FsiComm {
  void* user;
  int (*allreduce_sum)(void* user, double* host_vals, int32_t n);   /* in place, over all ranks                   */
  int (*halo_exchange)(void* user);                                 /* sendbuf_dev -> the peers' recvbuf_dev       */
} FsiComm;
/* dofs are user-layout dofs of this context.  num_owned_cells: cells [0, num_owned_cells) are counted in the
 * L2(Omega) norm of the Newton update by this rank.  ghost_dofs: every dof owned elsewhere (refreshed by the halo
 * exchange, zero in residual-type vectors); identity_dofs: the subset whose rows are incomplete here (the outermost
 * node layer).  With overlap layers (ghost rows that are complete) the preconditioner is restricted additive Schwarz:
 * the residual is refreshed into the overlap before the local solve, the owners' part of the result is kept.
 * Call before the first Jacobian assembly. */
int fsi_set_partition(FsiCtx* ctx, int64_t num_owned_cells, int64_t n_ghost, const int64_t* ghost_dofs,
                      int64_t n_identity, const int64_t* identity_dofs, int64_t n_send, const int64_t* send_dofs,
                      double* sendbuf_dev, double* recvbuf_dev, const FsiComm* comm);

/* Collectives issued by the library itself (the default of vasp_amd/partition.py on the nccl backend with more than one
 * rank; VASPFSI_RCCL=0 keeps the callbacks): after fsi_set_partition, hand the
 * library an RCCL communicator and it queues ncclAllReduce (Krylov coefficient vectors in device memory) and grouped
 * ncclSend / ncclRecv (halo) on its solver stream; the FsiComm callbacks are then no longer called.  Counterpart of the MPI
 * reductions inside the reference's solver run [REF docs/simulation.md:14-32; simulation_common.py:217-220].
 * fsi_rccl_unique_id: 128 bytes from ncclGetUniqueId, made by one rank and broadcast by the caller.  send_counts[p] /
 * recv_counts[p]: doubles exchanged with rank p, in the order of the partition's send / ghost lists (peers ascending).
 * RCCL is resolved with dlopen at the first call; FSI_ERR_DEVICE if it is not available.  id128 == NULL: destroy the
 * library's communicator and return to the FsiComm callbacks (what the caller does when any rank failed to set it up).
 * A RCCL call that fails later aborts the communicator (ncclCommAbort) and every further collective of the context returns
 * FSI_ERR_DEVICE at once, so that no rank waits for one that has left. */
int fsi_rccl_unique_id(void* id128);
int fsi_set_rccl(FsiCtx* ctx, const void* id128, int32_t rank, int32_t world, const int64_t* send_counts,
                 const int64_t* recv_counts);

/* ---- state / introspection (checkpoint, restart, parity dumps) --------------------------------------- */
/* which: 0 = dvp_["n"], 1 = dvp_["n-1"], 2 = last rhs b, 3 = last update du.  User layout, length ndof. */
int fsi_get_state(FsiCtx* ctx, int which, double* out);
int fsi_set_state(FsiCtx* ctx, int which, const double* in);
/* Replaces: the read loop of vasp-create-hdf5 / create_transformed_matrix that rebuilds a Function from one saved frame
 * [REF src/vasp/postprocessing/postprocessing_fenics/create_hdf5.py:139-160;
 *  src/vasp/postprocessing/postprocessing_h5py/postprocessing_h5py_common.py:154-409].  One frame of the Visualization files
 * into dvp_["n"] (which = 0) or dvp_["n-1"] (1): d and v are [n_nodes][3], p has n_nodes entries of which the first V are used,
 * all in the files' node order (vertices, then one node per edge).  Any of the three may be null: that field of the state is
 * left untouched.  n_nodes is N2 (save_deg 2: the values as they are) or V (save_deg 1: a mid-edge node takes 0.5 * (a + b) of
 * its edge's two vertices - the P1 field the reference's tools see in such a folder); anything else is FSI_ERR_INVALID with
 * both numbers in fsi_last_error.  The fields are staged in an existing work vector; the table of edge vertices is built at
 * the first save_deg 1 call and kept.  The copies have finished when the call returns: the caller's arrays may be unmapped.
 * Not for partitioned contexts. */
int fsi_set_frame(FsiCtx* ctx, int which, int64_t n_nodes, const double* d, const double* v, const double* p);
/* out[i] = state[dofs[i]] (user layout): what a hook needs of dvp_ on a patch (the inlet facets of
 * assemble(inner(v, n) * ds(inlet)) [REF src/vasp/simulations/simulation_common.py:276]) without the whole vector
 * crossing PCIe every time step. */
int fsi_get_values(FsiCtx* ctx, int which, int64_t n, const int64_t* dofs, double* out);
int64_t fsi_num_dofs(const FsiCtx* ctx);
int64_t fsi_matrix_nnz(const FsiCtx* ctx);
/* Free and total bytes of the context's device as the HIP runtime of the library sees them (hipMemGetInfo): how much of the
 * 288 GB one context of a given mesh takes, asked without a second runtime in the process. */
int fsi_device_memory(FsiCtx* ctx, int64_t* free_bytes, int64_t* total_bytes);
/* Copies the assembled matrix out in user-layout row/column numbering (CSR, rows sorted).  rowptr [ndof+1],
 * cols/vals [nnz].  Values are the un-equilibrated Jacobian after ident_zeros and bc.apply. */
int fsi_get_matrix(FsiCtx* ctx, int64_t* rowptr, int64_t* cols, double* vals);
/* z = M^-1 r: one application of the active preconditioner (precond 0: the field-split block preconditioner with its fixed
 * sweep counts - a fixed linear operator; 1: ILU(0)) to a residual in the user layout, as fsi_solve's Krylov method applies
 * it - the PCApply of a PETSc binding, and what the tests check linearity and the quality of the approximation on.  Single
 * contexts only. */
int fsi_apply_preconditioner(FsiCtx* ctx, const double* r, double* z);
/* y = A x with the device SpMV (user layout in/out). */
int fsi_spmv(FsiCtx* ctx, const double* x, double* y);

/* ---- per-step diagnostics of post_solve on the device --------------------------------------------------- */
/* Replaces: peval / print_probe_points / print_solid_probe_points [REF src/vasp/simulations/simulation_common.py:157-222].
 * Points are located once on the host (cell + barycentric coordinates, -1 = outside: the reference's +inf sentinel is
 * the caller's business); out[i] = d_x d_y d_z v_x v_y v_z p of dvp_["n"] at point i (P2 / P1 interpolation). */
int fsi_probe(FsiCtx* ctx, int64_t n, const int32_t* cells, const double* bary, double* out);
/* Replaces: the DG0 projections of calculate_and_print_flow_properties (:253-317) and compute_minimum_jacobian (:320-348):
 * out[0..3] = mean, min, max over the cells of the cell-mean |v|, and min over the cells of the cell-mean det(I + grad d).
 * After fsi_set_partition: over the cells this context owns (the caller combines the ranks with the owned-cell counts). */
int fsi_flow_stats(FsiCtx* ctx, double* out);

/* ---- post-processing kernels on the resident state ------------------------------------- */
/* Replaces the element loop of compute_stress_strain [REF src/vasp/postprocessing/postprocessing_fenics/
 * compute_stress_strain.py:188-263]: for each listed SOLID cell (index in the mesh handed to fsi_create) the DG1
 * coefficients (one per local vertex) of the L2-projected Cauchy stress 1/J F S F^T and Green-Lagrange strain E of
 * dvp_["n"]'s displacement, and of the projected largest principal value of each.
 * out[i][80] = TrueStress[4][3][3], GreenLagrangeStrain[4][3][3], MaxPrincipalStress[4], MaxPrincipalStrain[4]. */
int fsi_stress_strain(FsiCtx* ctx, int64_t n, const int32_t* cells, double* out);
/* Replaces Stress.__call__ of compute_hemodynamics [REF .../compute_hemodynamics.py:91-157]: tangential traction
 * Ft = F - (F.n) n, F = -2 mu sym(grad v) n, on the listed exterior facets (cell + local index of the opposite vertex),
 * projected with the surface mass matrix onto the DG1 space of each boundary cell; out[f][3][3] = value at the three
 * facet vertices (local vertices of the cell in ascending order without the opposite one) x component. */
int fsi_wall_shear_stress(FsiCtx* ctx, int64_t nf, const int32_t* facet_cells, const int32_t* facet_local, double mu,
                          double* out);

/* ---- hemodynamic indices accumulated on the device over a run (fsi_hemo.hip) --------------------------------- */
/* Replaces: the set-up of compute_hemodyanamics [REF src/vasp/postprocessing/postprocessing_fenics/compute_hemodynamics.py:
 * 160-255]: opens a session on the listed exterior facets (cell + local index of the opposite vertex, as
 * fsi_wall_shear_stress; a facet may not be listed twice) with dynamic viscosity mu > 0 and the time between two samples
 * dt_sample > 0.  Replaces any open session; the accumulators start at zero.  Not for partitioned contexts. */
int fsi_hemo_begin(FsiCtx* ctx, int64_t nf, const int32_t* facet_cells, const int32_t* facet_local, double mu,
                   double dt_sample);
/* Replaces: one iteration of the frame loop of compute_hemodyanamics [REF .../compute_hemodynamics.py:257-319]: tau of
 * dvp_["n"] (bit for bit fsi_wall_shear_stress) added to the sums behind the indices.  wss_out (nullable): tau, (nf,3,3)
 * as fsi_wall_shear_stress.  As in the reference, tau_prev is zero before the first sample: its TWSSG term is |tau_1| / dt.
 * FSI_ERR_INVALID without an open session. */
int fsi_hemo_sample(FsiCtx* ctx, double* wss_out);
/* Replaces: the closing arithmetic of compute_hemodyanamics [REF .../compute_hemodynamics.py:321-350]: with n samples,
 * per DG1 dof of the boundary mesh (facet f, vertex k -> 3 f + k; vertices in the order of fsi_wall_shear_stress)
 * out[5][nf][3] = TAWSS = sum|tau| / n, OSI = (1 - |sum tau / n| / TAWSS) / 2, RRT = 1 / |sum tau / n|, ECAP = OSI / TAWSS,
 * TWSSG = sum of the P1-projected |(tau - tau_prev) / dt_sample| / n; IEEE inf / NaN where a denominator vanishes.
 * *samples (nullable) = n.  FSI_ERR_INVALID without a session or before the first sample.  The session stays open. */
int fsi_hemo_indices(FsiCtx* ctx, double* out, int64_t* samples);
/* Replaces: nothing in the reference, whose frame loop [REF .../compute_hemodynamics.py:257-319] cannot be left and entered
 * again: the session's accumulator as it stands, for a checkpoint.  With nd = 3 nf DG1 dofs (facet f, vertex k -> 3 f + k)
 * acc_out[24 nf] = sum_tau[nd][3], tau_prev[nd][3], sum_mag[nd], sum_twssg[nd], one block after the other: the sum of tau,
 * the tau of the last sample, the sum of |tau| and the sum of the projected |(tau - tau_prev) / dt_sample|.  *samples
 * (nullable) = the number of samples.  Stream-ordered behind the samples taken; finished when the call returns.
 * FSI_ERR_INVALID without an open session, with a null acc_out and for a partitioned context. */
int fsi_hemo_export(FsiCtx* ctx, double* acc_out, int64_t* samples);
/* Replaces: the zero start of fsi_hemo_begin after a restart: acc[24 nf] (the layout of fsi_hemo_export, nf that of the
 * open session - the caller checks that the exporting session had the same facets) and samples >= 0 replace the session's
 * sums and its count, so the first TWSSG term of the continued run is formed with the tau_prev that was carried, not with
 * zero.  A run that samples k states, exports, imports into a new session on the same facets and samples the rest forms
 * the bits of an unsplit run.  FSI_ERR_INVALID without an open session, with a null acc, samples < 0 and for a partitioned
 * context; a refused call leaves the session as it was. */
int fsi_hemo_import(FsiCtx* ctx, const double* acc, int64_t samples);
/* Closes the session and frees its device memory (fsi_destroy does the same). */
int fsi_hemo_end(FsiCtx* ctx);

/* ---- solid stress / strain sampled on the device over a run (fsi_stress.hip) ------------------------------- */
/* Replaces: the set-up of compute_stress_strain [REF src/vasp/postprocessing/postprocessing_fenics/compute_stress_strain.py:
 * 160-187]: opens a session on n > 0 listed SOLID cells (indices in the mesh handed to fsi_create, as fsi_stress_strain),
 * checked and uploaded once.  Replaces any open session; the sums start at zero.  Not for partitioned contexts. */
int fsi_stress_begin(FsiCtx* ctx, int64_t n, const int32_t* cells);
/* Replaces: one iteration of the frame loop of compute_stress_strain [REF .../compute_stress_strain.py:188-250]: the frame
 * of dvp_["n"]'s displacement on the session's cells (bit for bit fsi_stress_strain), its eight principal values per cell
 * added to the session's sums (MPStress_avg / MPStrain_avg .vector().axpy(1.0, ...)).  frame_out (nullable): (n, 80) as
 * fsi_stress_strain.  FSI_ERR_INVALID without an open session. */
int fsi_stress_sample(FsiCtx* ctx, double* frame_out);
/* Replaces: the closing averages of compute_stress_strain [REF .../compute_stress_strain.py:255-257]: with n samples
 * out[2][ncell][4] = MaxPrincipalStress_avg, MaxPrincipalStrain_avg = the sums of the sampled DG1 coefficients / n.
 * *samples (nullable) = n.  FSI_ERR_INVALID without a session or before the first sample.  The session stays open. */
int fsi_stress_averages(FsiCtx* ctx, double* out, int64_t* samples);
/* Replaces: nothing in the reference (its frame loop [REF .../compute_stress_strain.py:188-250] runs in one go): the
 * session's sums for a checkpoint, sums_out[n][8] = per cell the sums of MaxPrincipalStress[4] and MaxPrincipalStrain[4]
 * over the samples, and *samples (nullable) their number.  Stream-ordered; finished when the call returns.
 * FSI_ERR_INVALID without an open session, with a null sums_out and for a partitioned context. */
int fsi_stress_export(FsiCtx* ctx, double* sums_out, int64_t* samples);
/* Replaces: the zero start of fsi_stress_begin after a restart: sums[n][8] (the layout of fsi_stress_export, n that of the
 * open session) and samples >= 0 replace the session's sums and its count.  FSI_ERR_INVALID without an open session, with
 * null sums, samples < 0 and for a partitioned context; a refused call leaves the session as it was. */
int fsi_stress_import(FsiCtx* ctx, const double* sums, int64_t samples);
/* Closes the session and frees its device memory (fsi_destroy does the same). */
int fsi_stress_end(FsiCtx* ctx);

/* ---- band-pass filtered fields and vibration amplitudes over a run (fsi_band.hip) -------------------------- */
/* One session per quantity (0 = d, 1 = v, 2 = p; 3 = strain, 4 = stress: fsi_band_begin_cells); all can be open together, and
 * beside the hemodynamics and the stress / strain session.  Rows are (node, component) pairs, row = ncomp * i + component for
 * the i-th listed node, ncomp = 3 for d / v and 1 for p - a fetched frame is the (n, ncomp) array a Visualization file holds.
 * All data are FP64. */
#define FSI_BAND_RAW 0
#define FSI_BAND_FILTERED 1
#define FSI_BAND_AMPLITUDE 2
#define FSI_BAND_MAGNITUDE 3
/* Replaces: create_transformed_matrix, the second pass over the Visualization files that builds the node x time matrix
 * [REF src/vasp/postprocessing/postprocessing_h5py/postprocessing_h5py_common.py:154-409].  Opens a session on n listed nodes
 * (P2 node ids for d / v, vertex ids for p); where nodes_b (nullable) is >= 0 the row is the mean of the two nodes' values (the
 * pressure at an edge node of the save_deg 2 output).  capacity: frames the history can take.  The bytes of the history, the
 * filtered series (capacity + 66 frames) and three work frames (fsi_band_room) are compared with the free device memory: if less than 1/16
 * of the device would stay free for the context, FSI_ERR_INVALID with both byte counts in fsi_last_error and nothing
 * allocated - no paging, no truncation.  Replaces an open session of the quantity; a refused call (node out of range,
 * capacity, device memory) leaves it as it was, its bytes counted as taken.  Not for partitioned contexts. */
int fsi_band_begin(FsiCtx* ctx, int32_t quantity, int64_t n, const int32_t* nodes, const int32_t* nodes_b, int64_t capacity);
/* The two tensor quantities of a band-pass session, opened by fsi_band_begin_cells (fsi_band_begin refuses them). */
#define FSI_BAND_STRAIN 3
#define FSI_BAND_STRESS 4
/* Replaces: create_transformed_matrix for quantity "strain" / "stress", the pass over StressStrain/GreenLagrangeStrain.h5 or
 * TrueStress.h5 that builds the six dof x time component matrices 11, 12, 22, 23, 33, 31 = entries 0, 1, 4, 5, 8, 6 of the nine
 * [REF src/vasp/postprocessing/postprocessing_h5py/postprocessing_h5py_common.py:198-260,349-354].  Opens the session of
 * quantity FSI_BAND_STRAIN or FSI_BAND_STRESS on n > 0 listed SOLID cells (indices as fsi_stress_begin; range and kind are
 * checked on the host before anything is uploaded).  A row is one component of one DG1 dof (local vertex a) of one listed
 * cell: row = (4 i + a) * 6 + component for the i-th cell, so a "node" of the other band calls is a dof 4 i + a and ncomp = 6:
 * 24 n rows, 4 n dofs.  The device-room refusal of fsi_band_begin applies to these counts.  Both quantities can be open
 * together and beside every other session.  Replaces an open session of the quantity; a refused call leaves it as it was.
 * Not for partitioned contexts.  The other fsi_band_* calls then serve the quantity:
 *   fsi_band_sample  one frame of compute_stress_strain [REF src/vasp/postprocessing/postprocessing_fenics/
 *                    compute_stress_strain.py:188-250] on the cells, the bits fsi_stress_sample puts into its frame;
 *   fsi_band_fetch   FSI_BAND_MAGNITUDE / max_out / argmax_out: per dof the largest principal value of the amplitude tensor
 *                    [[11,12,31],[12,22,23],[31,23,33]] by get_eig, exactly 0 where every entry is below 1e-8 in magnitude
 *                    [REF .../create_hi_pass_viz.py:295-314] (out[4 n]); with window 0 of the filtered tensor (:229-230);
 *   fsi_band_trace   refused: the reference writes no point traces for these quantities [REF .../create_hi_pass_viz.py:636-643];
 *   filter, filter_next, select, amplitude, export, import, end: as for d, v, p, on the 24 n rows. */
int fsi_band_begin_cells(FsiCtx* ctx, int32_t quantity, int64_t n, const int32_t* cells, int64_t capacity);
/* Replaces: reading one frame of <quantity>.h5 [REF .../postprocessing_h5py_common.py:154-409, its frame loop]: the session's rows of
 * dvp_["n"] go to the next frame of the history, stream-ordered behind the time step; the host does not wait.
 * FSI_ERR_INVALID when the history is full. */
int fsi_band_sample(FsiCtx* ctx, int32_t quantity);
/* Replaces: the node loop of create_hi_pass_viz [REF .../create_hi_pass_viz.py:190-215] around butter_bandpass_filter
 * [REF .../spectrograms.py:534-555]: scipy.signal.filtfilt(b, a, row) of every row over the frames recorded so far, in
 * scipy's arithmetic (odd extension by padlen, transposed direct form II, zi scaled by the first extended / last forward
 * sample), bit for bit.  ntaps = len(b) = len(a) in 2 .. 11, a[0] = 1, zi[ntaps - 1] = scipy.signal.lfilter_zi(b, a),
 * padlen <= 33 and < the number of frames (where scipy raises).  The raw history is kept: another band can follow. */
int fsi_band_filter(FsiCtx* ctx, int32_t quantity, int32_t ntaps, const double* b, const double* a, const double* zi,
                    int32_t padlen);
/* Replaces: the frame selection of create_transformed_matrix [REF .../postprocessing_h5py_common.py:285-307: start, stop and
 * stride over the Visualization files] and the start_t of the files that follow.  The filter, the amplitude, the fetches of
 * filtered / amplitude / magnitude frames and fsi_band_trace work on the recorded frames first, first + stride, ..., count of
 * them (frame k of these calls is recorded frame first + k * stride); a raw fetch keeps its index in the history.  Needs
 * stride >= 1 and first + (count - 1) * stride < the number of recorded frames; count = -1: as many as fit.  Invalidates the
 * filtered series and the amplitude.  fsi_band_sample resets the selection to every recorded frame.  Unlike the reference,
 * which drops the last frames of its range, every selected frame is kept. */
int fsi_band_select(FsiCtx* ctx, int32_t quantity, int64_t first, int64_t count, int64_t stride);
/* Replaces: one further band of the multiband loop of create_hi_pass_viz [REF .../create_hi_pass_viz.py:191-198], which
 * filters a row that is already filtered: y <- filtfilt(b, a, y) of every row of the filtered series, in the arithmetic of
 * fsi_band_filter, bit for bit, inside the series' own buffer (no device memory is allocated).  Arguments and checks as
 * fsi_band_filter; FSI_ERR_INVALID with "no filtered series (fsi_band_filter first)" when there is none, and when padlen
 * exceeds the previous stage's (every order-5 band-pass and band-stop has 33; put a longer filter first).  Invalidates the
 * amplitude; the raw history is kept. */
int fsi_band_filter_next(FsiCtx* ctx, int32_t quantity, int32_t ntaps, const double* b, const double* a, const double* zi,
                         int32_t padlen);
/* Replaces: calculate_windowed_rms [REF .../postprocessing_h5py_common.py:685-731] as create_hi_pass_viz uses it (:218-230):
 * selects the amplitude of the filtered series for the fetches that follow.  window > 0: sqrt(convolve(y^2, ones(window) /
 * window, "valid")) centred by (window - 1) / 2 frames, zero outside; window = 0: the filtered series itself (the reference's
 * low-pass case).  window may not exceed the number of frames. */
int fsi_band_amplitude(FsiCtx* ctx, int32_t quantity, int32_t window);
/* Replaces: compute_tke [REF src/vasp/postprocessing/log_plotter.py:928-989], which the reference applies to the probe points
 * of a log file: the phase-averaged (Reynolds) decomposition of every row of the session over the selected frames
 * (fsi_band_select sets the cycle range), n = C * period of them, C cycles of `period` frames.  With x[k] selected frame k:
 *   mean[j]  = (((+0.0 + x[j]) + x[period + j]) + ...) / C     for j < period, a true division;
 *   fluct[k] = x[k] - mean[k % period],
 * the reference's operations in its order, bit for bit.  The fluctuation becomes the session's filtered series of n frames
 * (padlen 0): fsi_band_fetch(FSI_BAND_FILTERED), fsi_band_trace(FSI_BAND_FILTERED), fsi_band_amplitude and the amplitude
 * fetches serve it - the windowed RMS of u' is the turbulence intensity.  The raw history is kept.  Needs period >= 1 and a
 * selected count that is a positive multiple of it, else FSI_ERR_INVALID naming both numbers.  The `period` frames of the
 * mean are an allocation of their own, 8 * period * rows bytes, under the room rule of fsi_band_begin: FSI_ERR_INVALID with
 * both byte counts when they do not fit beside the context's 1/16 of the device; nothing is paged (fsi_band_room does not
 * count them).  A refused call leaves the session as it was.  fsi_band_sample, _import, _select, _filter and _filter_next
 * invalidate the phase average and free the mean; fsi_band_end and fsi_destroy free it.  For d, v, p and, by rows, for the
 * two tensor quantities.  Not for partitioned contexts. */
int fsi_band_phase(FsiCtx* ctx, int32_t quantity, int64_t period);
#define FSI_PHASE_MEAN 0
#define FSI_PHASE_ENERGY 1
#define FSI_PHASE_ENERGY_CYCLE_MEAN 2
#define FSI_PHASE_ENERGY_TIME_MEAN 3
/* Replaces: the rest of compute_tke, 0.5 * (fx^2 + fy^2 + fz^2) [REF .../log_plotter.py:981-987], and
 * compute_average_over_cycles of it [REF .../log_plotter.py:902-925], for every node of the session after fsi_band_phase:
 *   FSI_PHASE_MEAN               frame < period: out[n][ncomp], the mean of phase `frame`;
 *   FSI_PHASE_ENERGY             frame < the selected count: out[n], e = 0.5 * ((fx fx + fy fy) + fz fz) of fluctuation frame
 *                                `frame` (for p 0.5 * (f f)), formed when fetched - no nodes x frames array is allocated;
 *   FSI_PHASE_ENERGY_CYCLE_MEAN  frame < period: out[n], the sum over the cycles c in order of e[c * period + frame], from
 *                                +0.0, divided by C (compute_average_over_cycles);
 *   FSI_PHASE_ENERGY_TIME_MEAN   frame == 0: out[n], the sum over all selected frames in order of e, from +0.0, divided by
 *                                their count (numpy.mean over the frames).
 * The three energies are refused for the tensor quantities (ncomp 6).  FSI_ERR_INVALID "no phase average (fsi_band_phase
 * first)" without one, for a frame out of range, a null out and a partitioned context. */
int fsi_band_phase_fetch(FsiCtx* ctx, int32_t quantity, int32_t what, int64_t frame, double* out);
/* Replaces: nothing in the reference, whose spectrogram reader only prepares for it [REF .../spectrograms.py:203]: the
 * spectral power index (SPI; Khan et al., J. Biomech. 2017) of every row of the session over the n selected RAW frames
 * (fsi_band_select), the fraction of the non-mean spectral power at or above a cut-off.  One call runs one slab of the nb
 * lowest bins bin0 .. bin0 + nb - 1 of the length-n DFT; Ct, St [n][nb] are the slab's cos / sin(2 pi j k / n), frame-major
 * (Ct[j * nb + b] for frame j, bin bin0 + b), window [n] or NULL for the boxcar.  With m the mean of a row over the frames,
 * added in frame order, Y[j] = window[j] * (x[j] - m) and X_k = sum_j Y[j] exp(-2 pi i j k / n), a row keeps three sums, each
 * added in a fixed order (fsi_spi.hip): L2 = sum_{1 <= k < kc} |X_k|^2 over the bins handed over so far, X0^2 = |X_0|^2 and
 * Q = sum_j Y[j]^2.  The slab with bin0 == 0 starts them (and forms m, X0^2 and Q); a slab with bin0 > 0 adds onto L2 and must
 * start where the slab before it ended, on the same selection, with the same window.  All slabs together hold bins 0 .. kc - 1,
 * kc - 1 <= (n - 1) / 2: a low bin lies below the Nyquist frequency.  The raw history and the filtered series are left alone.
 * The sums, the mean, the window and one slab's tables are allocations of the session's own, 8 * (5 rows + nodes + n + 2 n nb)
 * bytes, under the room rule of fsi_band_begin: FSI_ERR_INVALID with both byte counts when they do not fit beside the context's
 * 1/16 of the device, and where an allocation fails; nothing is paged.  FSI_ERR_INVALID also for the tensor quantities, fewer
 * than 2 selected frames, nb < 1, null tables, a bin at or above the Nyquist bin and a slab out of order; a refused call leaves
 * the session usable.  fsi_band_sample, _import and _select drop the index; fsi_band_end and fsi_destroy free it.  Not for
 * partitioned contexts. */
int fsi_band_spi(FsiCtx* ctx, int32_t quantity, const double* window, int64_t bin0, int64_t nb, const double* Ct, const double* St);
#define FSI_SPI_ROWS 0
#define FSI_SPI_NODES 1
#define FSI_SPI_SUMS 2
/* After fsi_band_spi, of the slabs run so far, with AC = n Q - X0^2 (all power but bin 0, two-sided, by Parseval) and
 * H = AC - 2 L2 (what lies at or above the cut-off):
 *   FSI_SPI_ROWS   out[rows]: H <= 0 ? 0 : H / AC - a row that is exactly constant (AC == 0) gives 0, a NaN stays NaN;
 *   FSI_SPI_NODES  out[n]: for a vector (sH <= 0 ? 0 : sH / sAC) with sH = (H_x + H_y) + H_z and sAC likewise - the index of
 *                  the summed power, invariant under a rotation of the axes; for the pressure the row's value;
 *   FSI_SPI_SUMS   out[3][rows]: L2, X0^2 and Q as they stand.
 * FSI_ERR_INVALID "no spectral power index (fsi_band_spi first)" without one, for a null out and a partitioned context. */
int fsi_band_spi_fetch(FsiCtx* ctx, int32_t quantity, int32_t what, double* out);
/* Replaces: nothing in the reference: the Gram matrix of the snapshot proper orthogonal decomposition (POD) of the session's
 * n >= 2 selected frames (fsi_pod.hip).  series: FSI_RATE_RAW the selected raw frames through the selection's stride,
 * FSI_RATE_SERIES the filtered series or the fluctuation, whichever stands; FSI_RATE_PHASE_MEAN is refused.  node_weights: a
 * host array of one value >= 0 and finite per node of the session, or NULL for 1; checked on the host, the refusal names the
 * first offending node.  With m[r] the mean of row r over the n frames, added in frame order (k_spec_mean), y_j = x_j - m and
 * a_j[r] = w_r y_j[r] rounded once (NULL: y_j itself, no product):
 *   G[i][j] = sum_r a_i[r] y_j[r],
 * formed for i <= j and mirrored, so G is symmetric bit for bit.  The rows are added in slabs of 6144 rows, four rows at a time
 * in ascending order inside a slab, the slabs in ascending order: an order that depends on the numbers of rows and frames
 * alone; no atomics, the same call gives the same bits.  A sum over the rows: one NaN or inf in the history makes every entry
 * of G non-finite.  The call replaces a decomposition that stood, its modes included.  G, the slabs' partial sums, the mean and
 * the weights are allocations of the session's own under the room rule of the begin calls: FSI_ERR_INVALID with both byte
 * counts where they do not fit beside 1/16 of the device; a refused call changes nothing.  FSI_ERR_INVALID also without a
 * session, for the tensor quantities (ncomp 6), a partitioned context, fewer than 2 selected frames (more than 16384),
 * FSI_RATE_SERIES without a series.  fsi_band_sample, _import and _select drop the decomposition; fsi_band_filter,
 * _filter_next and _phase drop one of the series and leave one of the raw frames; fsi_band_end and fsi_destroy free it. */
int fsi_band_pod_gram(FsiCtx* ctx, int32_t quantity, int32_t series, const double* node_weights);
/* Replaces: nothing in the reference: the modes of the decomposition whose Gram matrix stands (fsi_band_pod_gram),
 *   Phi_m[r] = sum_j table[j * nmodes + m] * y_j[r],   m < nmodes, 1 <= nmodes <= 64,
 * table[frames][nmodes] from the host - for orthonormal modes T[j][m] = V[j][m] / sqrt(lambda_m) of G V = V diag(lambda) - on
 * the source and the mean the Gram matrix was formed on; the frames are added four at a time in ascending order.  Replaces the
 * modes that stood.  The table and the modes are allocations of the session's own under the room rule.  FSI_ERR_INVALID
 * "no Gram matrix (fsi_band_pod_gram first)" without one, for nmodes out of range, a null table, a partitioned context. */
int fsi_band_pod_modes(FsiCtx* ctx, int32_t quantity, int32_t nmodes, const double* table);
#define FSI_POD_GRAM 0
#define FSI_POD_MEAN 1
#define FSI_POD_MODE 2
/* Replaces: nothing in the reference: what the decomposition holds, to the host.
 *   FSI_POD_GRAM  out[n][n], the Gram matrix (index is not read);
 *   FSI_POD_MEAN  out[nodes][ncomp], the mean the frames were taken about (index is not read);
 *   FSI_POD_MODE  out[nodes][ncomp], mode `index` of fsi_band_pod_modes.
 * FSI_ERR_INVALID "no Gram matrix (fsi_band_pod_gram first)" without one, "no modes (fsi_band_pod_modes first)" for a mode
 * without them, for an index out of range, a null out and a partitioned context. */
int fsi_band_pod_fetch(FsiCtx* ctx, int32_t quantity, int32_t what, int64_t index, double* out);
/* Replaces: nothing in the reference; VaMPy's metrics on an FSI run.  Attaches n > 0 mesh cells to the open session of
 * quantity 0 (d) or 1 (v) (fsi_band_begin), for fsi_band_cell_rate.  Every one of a cell's ten P2 nodes must be a node of the
 * session whose row is the node's own value (nodes_b < 0); of a node listed twice the first occurrence is used.  The range of
 * the cells is checked on the host before anything is uploaded; a cell with a node the session does not hold is
 * FSI_ERR_INVALID naming the first such cell and node.  Uploaded: conn[n][10] (indices into the session's nodes, local order:
 * the vertices, then the edges {2,3},{1,3},{1,2},{0,3},{0,2},{0,1}) and gl[n][4][3], the gradients of the cells' barycentric
 * coordinates in the undeformed geometry, as wss_dg1_cell and the reference's hemodynamics take them - 136 bytes per cell - and
 * a result out[n]; under the room rule of fsi_band_begin: FSI_ERR_INVALID with both byte counts when the 144 n bytes do not fit
 * beside the context's 1/16 of the device.  grad_out (nullable): [n][4][3], the gradients the kernel will use, so that a host
 * twin works from the same bits.  A second call replaces the list; a refused call leaves the list that stands in place;
 * fsi_band_begin, fsi_band_end and fsi_destroy free it; fsi_band_sample, _import, _select, _filter, _filter_next and _phase
 * leave it alone.  Refused for p, the tensor quantities, a quantity without a session and partitioned contexts. */
int fsi_band_cells(FsiCtx* ctx, int32_t quantity, int64_t n, const int32_t* cells, double* grad_out);
#define FSI_RATE_RAW 0
#define FSI_RATE_SERIES 1
#define FSI_RATE_PHASE_MEAN 2
/* Replaces: nothing in the reference; VaMPy's metrics on an FSI run.  out[n], per cell of fsi_band_cells
 *   out[c] = (((+0.0 + r[first]) + r[first + step]) + ...) / count,     count terms in frame order, a true division,
 * r[k] being the exact mean over the cell of 2 S:S, S = sym(grad w), of frame k of a series w of the session:
 *   FSI_RATE_RAW         the selected frames of the history, through the selection's stride (fsi_band_select);
 *   FSI_RATE_SERIES      the filtered series (fsi_band_filter, _filter_next) or the fluctuation (fsi_band_phase), whichever
 *                        the session holds;
 *   FSI_RATE_PHASE_MEAN  the `period` frames of the phase mean (fsi_band_phase).
 * With G_t = grad w at vertex t (the gradient of a P2 field is linear on the cell) and S_t = 0.5 (G_t + G_t^T):
 * r = 0.1 * (sum_t S_t:S_t + (sum_t S_t):(sum_t S_t)).  FP64 without contraction, bit-equal to hi_pass.cell_rate; count = 1
 * gives the frame's own bits; NaN and inf propagate, nothing is clamped.  One frame: (k, 1, 1); the time mean: (0, 1, n); the
 * cycle mean at phase j: (j, period, C).  sqrt(out) of the velocity is the strain rate |S| = sqrt(2 S:S), nu * out the viscous
 * dissipation.  FSI_ERR_INVALID, naming what is missing: no cell list (fsi_band_cells first), no filtered series
 * (fsi_band_filter or fsi_band_phase first), no phase average (fsi_band_phase first), step < 1 or count < 1, a last frame
 * outside the series, out NULL; p, the tensor quantities, a quantity without a session and partitioned contexts. */
int fsi_band_cell_rate(FsiCtx* ctx, int32_t quantity, int32_t series, int64_t first, int64_t step, int64_t count, double* out);
/* Replaces: nothing in the reference; VaMPy's metrics on an FSI run.  fsi_band_cell_rate in the current configuration
 * x = X + d(X) of an ALE run: quantity, series, first, step and count as there, on the session of `quantity` and its cell list
 * (fsi_band_cells); the geometry is the displacement the session of quantity 0 (d) holds on the same nodes and frames:
 *   FSI_RATE_RAW, FSI_RATE_SERIES  the recorded (raw) d frame at the absolute index sel_first + (first + k step) sel_stride of
 *                                  the selection of the session of `quantity` - the d session's own selection does not matter;
 *   FSI_RATE_PHASE_MEAN            the d session's phase mean of the same phase (fsi_band_phase with the same period on the
 *                                  same selection).
 * With G_t and D_t the vertex gradients of the series' frame and of d in the undeformed geometry, at the four points of the
 * degree-2 interior rule (weight a = 0.5854101966249685 on vertex q, b = 0.1381966011250105 on the others):
 * G_q = b (sum_t G_t) + (a - b) G_q and D_q likewise, F_q = I + D_q, J_q = det F_q, L_q = G_q adj(F_q) / J_q,
 * S_q = 0.5 (L_q + L_q^T), e_q = 2 S_q:S_q and r = (sum_q J_q e_q) / (sum_q J_q), the mean over the deformed cell.  Per cell:
 *   rate_out[c]          (((+0.0 + r[first]) + r[first + step]) + ...) / count, as fsi_band_cell_rate;
 *   volume_ratio_out[c]  (nullable) the same ordered mean of 0.25 sum_q J_q, the deformed cell's volume over the undeformed;
 *   min_jacobian_out[c]  (nullable) the smallest J_q over the frames and points: m = +inf, m = (J_q < m) ? J_q : m, so a NaN
 *                        never replaces m.
 * FP64 without contraction, bit-equal to hi_pass.cell_rate_current.  Nothing is clamped: J_q = 0 gives IEEE inf or NaN in the
 * rate, a negative J_q is carried through, a NaN in a node reaches only the cells that touch it.  The two further result
 * buffers of n doubles are allocated at the first call under the room rule of fsi_band_begin and freed with the cell list.
 * FSI_ERR_INVALID, naming what is missing: every refusal of fsi_band_cell_rate (rate_out NULL among them); the d session is not
 * open, lists other nodes than the session of `quantity` or has recorded another number of frames; for the phase mean, the d
 * session has no phase average, or one of another period or over another selection; partitioned contexts.  A refused call
 * leaves the session as it was. */
int fsi_band_cell_rate_current(FsiCtx* ctx, int32_t quantity, int32_t series, int64_t first, int64_t step, int64_t count,
                               double* rate_out, double* volume_ratio_out, double* min_jacobian_out);
/* Replaces: nothing in the reference.  One weight per cell of the list fsi_band_cells attached to the session of quantity 0 (d)
 * or 1 (v): weights[n], host doubles in the list's order (the cell volumes, for a bulk integral), copied to the device for the
 * sums of fsi_band_cell_vortex; NULL drops them.  A call to fsi_band_cells drops them too: the list changed.  The buffer of n
 * doubles is allocated at the first call under the room rule of fsi_band_begin and freed with the cell list.  FSI_ERR_INVALID
 * "no cell list (fsi_band_cells first)" without one; p, the tensor quantities, a quantity without a session and partitioned
 * contexts. */
int fsi_band_cell_weights(FsiCtx* ctx, int32_t quantity, const double* weights);
#define FSI_VORTEX_Q 0
#define FSI_VORTEX_ENSTROPHY 1
#define FSI_VORTEX_HELICITY 2
#define FSI_VORTEX_ABS_HELICITY 3
#define FSI_VORTEX_SPEED2 4
#define FSI_VORTEX_FIELDS 5
/* Replaces: nothing in the reference.  Vortex identification on the cells of fsi_band_cells: quantity, series, first, step and
 * count as fsi_band_cell_rate takes them.  cells_out[5][n] (nullable), per field f and cell c
 *   cells_out[f][c] = (((+0.0 + r_f[first]) + r_f[first + step]) + ...) / count,     count terms in frame order, a true division,
 * r_f[k] being an exact mean over the cell of frame k of the series w, with G_t = grad w at vertex t (the gradient of a P2 field
 * is linear on the cell, so mean(f h) = 0.05 (sum_t f_t h_t + (sum_t f_t)(sum_t h_t)) for entries f, h of it) and
 * omega_t = (G_t[2][1] - G_t[1][2], G_t[0][2] - G_t[2][0], G_t[1][0] - G_t[0][1]):
 *   FSI_VORTEX_Q             -0.5 sum_ij mean(G_ij G_ji) = 0.5 (|Omega|^2 - |S|^2), the Q-criterion;
 *   FSI_VORTEX_ENSTROPHY     mean(|omega|^2);
 *   FSI_VORTEX_HELICITY      mean(w . omega) = sum_t sum_i (sum_a M[a][t] w[a][i]) omega_t[i], 60 M[a][t] = 0 / -1 for a vertex
 *                            a == t / a != t, 4 / 2 for an edge that has / has not vertex t;
 *   FSI_VORTEX_ABS_HELICITY  |FSI_VORTEX_HELICITY| of the frame: the absolute value of the cell mean, not the cell mean of
 *                            |w . omega|;
 *   FSI_VORTEX_SPEED2        mean(|w|^2) = sum_i sum_a w[a][i] (sum_b MM[a][b] w[b][i]), MM the P2 mass matrix over |K|.
 * sums_out[5] (nullable): sums_out[f] = sum_c weights[c] * cells_out[f][c] with the weights of fsi_band_cell_weights, in a fixed
 * bracket: p_c = weights[c] * value (one rounding); per 256 consecutive cells of the list (+0.0 past n) and inside each 64 of
 * them a balanced tree over adjacent pairs, the four sums of 64 as ((s0 + s1) + s2) + s3, and the groups of 256 from +0.0 in
 * ascending order.  FP64 without contraction, bit-equal to hi_pass.cell_vortex and hi_pass.cell_wsum; count = 1 gives the
 * frame's own bits; NaN and inf propagate, nothing is clamped.  The gradients are those of the undeformed mesh
 * (fsi_band_cell_vortex_current: those of the current configuration).  The result
 * and partial buffers (5 n + 5 ceil(n / 256) + 5 doubles) are allocated at the first call under the room rule of fsi_band_begin
 * and freed with the cell list.  FSI_ERR_INVALID, naming what is missing: every refusal of fsi_band_cell_rate; both outputs
 * NULL; sums_out without weights (fsi_band_cell_weights first); partitioned contexts.  A refused call changes nothing. */
int fsi_band_cell_vortex(FsiCtx* ctx, int32_t quantity, int32_t series, int64_t first, int64_t step, int64_t count,
                         double* cells_out, double* sums_out);
#define FSI_VORTEX_VOLUME_RATIO 5
#define FSI_VORTEX_CURRENT_FIELDS 6
/* Replaces: nothing in the reference.  fsi_band_cell_vortex in the current configuration x = X + d(X) of an ALE run: quantity,
 * series, first, step and count as there, on the session of `quantity`, its cell list and its weights; the geometry is the
 * displacement the session of quantity 0 (d) holds on the same nodes and frames, paired as fsi_band_cell_rate_current pairs it:
 *   FSI_RATE_RAW, FSI_RATE_SERIES  the recorded (raw) d frame at the absolute index sel_first + (first + k step) sel_stride of
 *                                  the selection of the session of `quantity` - the d session's own selection does not matter;
 *   FSI_RATE_PHASE_MEAN            the d session's phase mean of the same phase (the same period on the same selection).
 * With G_t and D_t the vertex gradients of the series' frame w and of d in the undeformed geometry, at the 14 points p of the
 * positive interior rule of degree 5 (barycentrics lam_p, weights om_p, sum_p om_p = 1):
 *   p = 0..3    1 - 3 a1 on vertex p, a1 = 0.31088591926330060980 on the other three       om = 0.11268792571801585080
 *   p = 4..7    the same with a2 = 0.092735250310891226402, vertex p - 4                    om = 0.073493043116361949544
 *   p = 8..13   0.5 - b on the two ends of local edge p - 8, b = 0.045503704125649649492
 *               on the other two                                                            om = 0.042546020777081466438
 * G_p = sum_t lam_p[t] G_t and D_p likewise (exact: the gradients are linear on the cell), F_p = I + D_p, A_p = adj F_p,
 * J_p = det F_p, L_p = (G_p A_p) (1 / J_p), v_p = sum_a N_a(lam_p) w[a] with the P2 basis N_a = lam_a (2 lam_a - 1) at a
 * vertex and 4 lam_r lam_s on the edge {r, s}, omega_p = (L_p[2][1] - L_p[1][2], L_p[0][2] - L_p[2][0], L_p[1][0] - L_p[0][1]),
 * and the integrands
 *   f_0 = -0.5 sum_ij L_ij L_ji    f_1 = |omega_p|^2    f_2 = v_p . omega_p    f_4 = |v_p|^2.
 * Per frame Jbar = sum_p om_p J_p - for a P2 displacement the exact volume of the deformed cell over the undeformed -, the
 * numerators n_f = sum_p (om_p J_p) f_p, n_3 = |n_2|, and the means over the deformed cell r_f = n_f / Jbar, r_3 = |r_2|.  With
 * d = 0 the rule is exact for all of them and r_f is field f of fsi_band_cell_vortex to rounding.
 * cells_out[6][n] (nullable): per cell the means over the frames - (((+0.0 + x[first]) + x[first + step]) + ...) / count, a
 * true division - of r_0 .. r_4 (FSI_VORTEX_Q .. FSI_VORTEX_SPEED2) and, as FSI_VORTEX_VOLUME_RATIO, of Jbar.
 * sums_out[6] (nullable): sums_out[f] = sum_c weights[c] * m_f[c] in the bracket of fsi_band_cell_vortex, m_f the same means
 * over the frames of the numerators n_0 .. n_4 and of Jbar: integrals per undeformed volume, so that with the undeformed cell
 * volumes as weights and count = 1 they are the frame's integrals over the current fluid domain and sums_out[5] is its current
 * volume.  FP64 without contraction, bit-equal to hi_pass.cell_vortex_current and hi_pass.cell_wsum.  Nothing is clamped:
 * J_p = 0 gives IEEE inf or NaN, a negative J_p is carried through, a NaN in a node reaches only the cells that touch it.  The
 * result and partial buffers (12 n + 6 ceil(n / 256) + 6 doubles) are allocated at the first call under the room rule of
 * fsi_band_begin and freed with the cell list.  FSI_ERR_INVALID, naming what is missing: every refusal of fsi_band_cell_vortex
 * and every refusal of fsi_band_cell_rate_current about the session of d, under this function's name.  A refused call changes
 * nothing. */
int fsi_band_cell_vortex_current(FsiCtx* ctx, int32_t quantity, int32_t series, int64_t first, int64_t step, int64_t count,
                                 double* cells_out, double* sums_out);
/* Replaces: the "Saving data" loops of create_hi_pass_viz [REF .../create_hi_pass_viz.py:233-245,327-341,377-390]: one frame
 * of the raw history, the filtered series or its amplitude (out[n][ncomp]), or of the amplitude's magnitude over the
 * components (out[n]; for p the amplitude itself).  For the last two, max_out / argmax_out (nullable) receive the largest
 * magnitude of the frame and the first node that has it (numpy.argmax).  out is nullable.  Amplitude frames are computed
 * when fetched, cheapest in ascending order; a frame's value does not depend on the order. */
int fsi_band_fetch(FsiCtx* ctx, int32_t quantity, int32_t what, int64_t frame, double* out, double* max_out,
                   int64_t* argmax_out);
/* Replaces: create_point_trace [REF .../postprocessing_h5py_common.py:470-483] and the frames * full-frame reads behind it:
 * the time series of npoints listed nodes over the selected frames, from the raw history (what = FSI_BAND_RAW) or the
 * filtered series (FSI_BAND_FILTERED), in one copy.  points[npoints]: indices into the session's node list (0 <= . < n, else
 * FSI_ERR_INVALID "node out of range"; a node may be listed twice).  out[npoints][frames][1 + ncomp]: the magnitude
 * sqrt((x x + y y) + z z) first (for p the value itself), then the ncomp values. */
int fsi_band_trace(FsiCtx* ctx, int32_t quantity, int32_t what, int64_t npoints, const int32_t* points, double* out);
/* Replaces: reading frames first .. first + count - 1 of <quantity>.h5 back [REF .../postprocessing_h5py_common.py:154-409],
 * for a checkpoint: out[count][n][ncomp], the raw history's frames in one copy (the history is frame-major).  first is an
 * index into the history, as in a raw fsi_band_fetch, whatever fsi_band_select holds.  Stream-ordered behind the frames
 * sampled; finished when the call returns.  FSI_ERR_INVALID unless first >= 0, count >= 1 and first + count <= the recorded
 * frames, with a null out, without an open session and for a partitioned context. */
int fsi_band_export(FsiCtx* ctx, int32_t quantity, int64_t first, int64_t count, double* out);
/* Replaces: count calls of fsi_band_sample after a restart: frames[count][n][ncomp] (what fsi_band_export gave, of a
 * session on the same nodes) are appended to the history - the recorded frames grow by count, the filtered series and the
 * amplitude are invalidated and the selection is reset to every recorded frame.  The filter, the amplitude and the traces
 * of the continued history are those of one that was sampled in one go, bit for bit.  FSI_ERR_INVALID when the recorded
 * frames + count exceed the capacity, with count < 1 or null frames, without an open session and for a partitioned context;
 * a refused call leaves the session as it was. */
int fsi_band_import(FsiCtx* ctx, int32_t quantity, int64_t count, const double* frames);
/* Replaces: the sizing a user of create_transformed_matrix does by hand before the node x time matrix is allocated in host
 * memory [REF .../postprocessing_h5py_common.py:309-321]: the two byte counts fsi_band_begin and fsi_band_begin_cells compare
 * for a session of `rows` rows (3 per node for d / v, 1 for p, 24 per cell for strain / stress) and `capacity` frames.
 * *need: the history, the filtered series (capacity + 66 frames), one frame each of running sums, amplitudes and magnitudes
 * and the row lists, 8 * rows * (2 * capacity + 70) bytes; *available: the free device memory less the 1/16 of the device
 * that stays with the context.  A begin call is refused exactly when need > available.  Nothing is allocated. */
int fsi_band_room(FsiCtx* ctx, int64_t rows, int64_t capacity, double* need, double* available);
/* Replaces: rms_magnitude, the node x time matrix of amplitude magnitudes create_hi_pass_viz keeps in host memory for its
 * table [REF .../create_hi_pass_viz.py:244,341,370-376], for a quantity whose rows go through the band-pass sessions in
 * strips: board[frame][node], FP64, 8 * nodes * frames bytes, one per context.  Refused like a session when it does not fit
 * beside the context's 1/16 of the device: FSI_ERR_INVALID with both byte counts in fsi_last_error, nothing allocated, an
 * open board left as it was.  Replaces an open board and detaches every session.  Not for partitioned contexts. */
int fsi_board_begin(FsiCtx* ctx, int64_t nodes, int64_t frames);
/* Frees the board and detaches every session (fsi_destroy does the same). */
int fsi_board_end(FsiCtx* ctx);
/* Replaces: the row range a strip of nodes takes in rms_magnitude [REF .../create_hi_pass_viz.py:341]: ties the open session of
 * `quantity` to the board at node offset node0 (0 <= node0, node0 + the session's nodes <= the board's), or detaches it
 * with node0 = -1.  From then on every fsi_band_fetch of FSI_BAND_AMPLITUDE or FSI_BAND_MAGNITUDE of frame k also stores the
 * frame's magnitudes - what the fetch forms for max_out / argmax_out - into board[k][node0 .. node0 + n); k must be a frame
 * of the board.  What a fetch returns does not change.  FSI_ERR_INVALID without a board, without a session, for a range
 * outside the board and for a partitioned context. */
int fsi_band_board_attach(FsiCtx* ctx, int32_t quantity, int64_t node0);
/* Replaces: the eleven np.percentile calls, the np.max and the np.argmax per frame of the amplitude table
 * [REF .../create_hi_pass_viz.py:377-390].  For board frames first .. first + count - 1: values[count][nranks], the order
 * statistics of the frame's magnitudes at the zero-based ranks[nranks] (rank 0 the smallest; 0 <= rank < nodes; a rank may be
 * listed twice; at most 32 distinct ranks) - a percentile is an interpolation of two neighbouring ones, formed by the caller
 * -, nan_counts[count], the frame's NaNs (they order behind +inf, as numpy sorts them), max_out[count] and argmax_out[count],
 * the largest magnitude and the first node that has it.  Exact: a radix select on the bits, integer counts only; the same
 * call returns the same bits.  FSI_ERR_INVALID, with nothing written, without a board, for frames outside it, a rank out of
 * range, null pointers and a partitioned context. */
int fsi_board_table(FsiCtx* ctx, int64_t first, int64_t count, int32_t nranks, const int64_t* ranks, double* values,
                    int64_t* nan_counts, double* max_out, int64_t* argmax_out);
/* Replaces: np.percentile's partition of one array [REF .../create_hi_pass_viz.py:379-389] for a caller's own data: the
 * selection of fsi_board_table on values[n] of the host, copied to the device, selected there and copied back.  out[nranks]:
 * the elements of rank ranks[k] in ascending order (-0 orders below +0, subnormals as their values); *nan_count: the NaNs.
 * FSI_ERR_INVALID, with nothing written, unless 1 <= n < 2^32, for a rank out of range, more than 32 distinct ranks, null
 * pointers and a partitioned context. */
int fsi_order_statistics(FsiCtx* ctx, int64_t n, const double* values, int32_t nranks, const int64_t* ranks, double* out,
                         int64_t* nan_count);
/* Closes the session of the quantity and frees its device memory (fsi_destroy does the same). */
int fsi_band_end(FsiCtx* ctx, int32_t quantity);

/* ---- average spectrograms and power spectra over a run (fsi_spec.hip) -------------------------------------- */
/* One session per quantity (0 = d, 1 = v, 2 = p, 3 = the wall shear stress, opened by fsi_spec_begin_wss), with a history of its
 * own on a node list of its own: it can be open beside
 * the band-pass session of the same quantity, and beside every other session.  A row is one time series: one component of a
 * listed node, its three components stacked (row = component * n + i), or the magnitude of the vector, taken when the frame is
 * recorded.  The pressure has one component: ncomp_mode is ignored for it.  All data are FP64. */
#define FSI_SPEC_X 0
#define FSI_SPEC_Y 1
#define FSI_SPEC_Z 2
#define FSI_SPEC_ALL 3
#define FSI_SPEC_MAG 4
#define FSI_SPEC_WSS 3 /* the quantity of fsi_spec_begin_wss */
#define FSI_SPEC_SPECTRUM 0 /* power scaled by 1 / sum(w)^2 */
#define FSI_SPEC_DENSITY 1  /* power scaled by 1 / (fs sum(w^2)) */
/* Replaces: read_spectrogram_data's pass over the Visualization files into <quantity>_<component>.npz and its selection of the
 * sampled rows [REF src/vasp/postprocessing/postprocessing_h5py/spectrograms.py:291-329; postprocessing_h5py_common.py:154-409].
 * nodes / nodes_b as in fsi_band_begin (a node may be listed more than once: the reference draws with replacement).  The bytes
 * of the raw and the filtered history (capacity and capacity + 66 frames) and of what the transforms allocate at the end (64 bins
 * of a periodogram's tables, the means of capacity / 4 segments) are compared with the free device memory as in
 * fsi_band_begin: FSI_ERR_INVALID with both byte counts, nothing allocated.  Replaces an open session of the quantity; a
 * refused call leaves it as it was, its bytes counted as taken.  Not for partitioned contexts. */
int fsi_spec_begin(FsiCtx* ctx, int32_t quantity, int64_t n, const int32_t* nodes, const int32_t* nodes_b, int32_t ncomp_mode,
                   int64_t capacity);
/* Replaces: the selection of a range of rows of the sampled matrix, df.iloc[r0:r1] [REF .../spectrograms.py:291-329], for a
 * history that goes through the session in strips of rows: a session on nrows listed ROWS instead of nodes.  Row r is
 * component comps[r] (0 = x, 1 = y, 2 = z) of nodes[r], or its mean with that of nodes_b[r] where nodes_b is given and
 * nodes_b[r] >= 0; for the pressure comps is ignored and may be null.  With FSI_SPEC_ALL the rows of fsi_spec_begin are
 * component-major (row = c * n + i), so a range of them can cross a component boundary: this call takes any such range.  A
 * strip of magnitudes is a sub-list of nodes and keeps fsi_spec_begin.  Recording, filtering, fetch, export, import and the
 * transforms work as for any session.  Checks, the device-room refusal (fsi_spec_room) and the treatment of an open session
 * as in fsi_spec_begin; FSI_ERR_INVALID also for a component outside 0 .. 2 and for null comps with d or v.  Not for
 * partitioned contexts. */
int fsi_spec_begin_rows(FsiCtx* ctx, int32_t quantity, int64_t nrows, const int32_t* nodes, const int32_t* nodes_b,
                        const int32_t* comps, int64_t capacity);
/* Replaces: the second tool run (vasp-compute-hemo), the pass of read_spectrogram_data over its WSS.h5 into a host matrix and the
 * selection of the sampled rows [REF src/vasp/postprocessing/postprocessing_fenics/compute_hemodynamics.py:160-372;
 * .../spectrograms.py:291-329 with quantity "wss"]: the session of quantity FSI_SPEC_WSS, whose rows are the wall shear stress at
 * DG1 dofs of the fluid's boundary mesh, formed on the device at every recorded frame by the arithmetic of
 * fsi_wall_shear_stress and fsi_hemo_sample (the same bits).  facet_cells[nf] / facet_local[nf]: ALL exterior facets of the
 * fluid, as for fsi_hemo_begin - the projection on a cell couples all of that cell's exterior facets, so the list must be the
 * full one even when one dof is sampled; mu: the dynamic viscosity.  Dof 3 f + k is vertex k of facet f (the local vertices of
 * its cell without facet_local[f], ascending).  Row r is component comps[r] (0 = x, 1 = y, 2 = z, 3 = the magnitude
 * sqrt((x x + y y) + z z), taken when the frame is recorded) of dof dofs[r], 0 <= dofs[r] < 3 nf; a dof may be listed more than
 * once.  The call is row-based: a strip of a longer row list is a sub-list and needs no second entry point.  The device-room
 * refusal is that of fsi_spec_begin_rows, a magnitude row counted as in fsi_spec_room(..., magnitude = 1).  FSI_ERR_INVALID with
 * one line in fsi_last_error and nothing allocated: a partitioned context, nf < 1, mu <= 0, a facet's cell or local index out of
 * range, a facet of a non-fluid cell, a facet listed twice, a dof or a component out of range, nrows < 1, capacity < 1.
 * Replaces an open session of the quantity; a refused call leaves it as it was.  fsi_spec_sample, _filter, _fetch, the
 * transforms, _export, _import and _end serve quantity 3 as the others. */
int fsi_spec_begin_wss(FsiCtx* ctx, int64_t nf, const int32_t* facet_cells, const int32_t* facet_local, double mu, int64_t nrows,
                       const int32_t* dofs, const int32_t* comps, int64_t capacity);
/* Replaces: the sizing a user of read_spectrogram_data does by hand before the row x time matrix is read into host memory
 * [REF .../spectrograms.py:291-329]: the two byte counts fsi_spec_begin and fsi_spec_begin_rows compare for a session of
 * `rows` rows (`magnitude` != 0: rows of FSI_SPEC_MAG, which sample three entries each) and `capacity` frames.  *need: the raw
 * and the filtered history (capacity and capacity + 66 frames), the row lists, 64 bins of a periodogram's tables over capacity
 * frames and the means of capacity / 4 segments, about 8 * rows * (2.25 * capacity + 68) bytes; *available: the free device
 * memory less the 1/16 of the device that stays with the context.  A begin call is refused exactly when need > available.
 * Nothing is allocated. */
int fsi_spec_room(FsiCtx* ctx, int64_t rows, int32_t magnitude, int64_t capacity, double* need, double* available);
/* Replaces: reading one frame of <quantity>.h5 [REF .../postprocessing_h5py_common.py:154-409, its frame loop]: the session's rows
 * of dvp_["n"] (or their magnitude) go to the next frame of the history, stream-ordered; the host does not wait.
 * FSI_ERR_INVALID when the history is full. */
int fsi_spec_sample(FsiCtx* ctx, int32_t quantity);
/* Replaces: filter_time_data [REF .../spectrograms.py:558-583]: scipy.signal.filtfilt(b, a, row) of every row, by the band-pass
 * session's kernel (bit for bit; arguments as fsi_band_filter; the reference's high-pass is butter(6, lowcut / (fs / 2),
 * "highpass"): 7 coefficients, padlen 21), and selects the filtered series as the source of the transforms that follow.
 * ntaps = 0 (b, a, zi ignored) selects the raw series.  Recording a frame selects the raw series again. */
int fsi_spec_filter(FsiCtx* ctx, int32_t quantity, int32_t ntaps, const double* b, const double* a, const double* zi,
                    int32_t padlen);
/* Replaces: df.iloc[row] of the sampled matrix [REF .../spectrograms.py:320-321]: out[rows] = one frame of the raw (filtered =
 * 0) or of the filtered history. */
int fsi_spec_fetch(FsiCtx* ctx, int32_t quantity, int32_t filtered, int64_t frame, double* out);
/* Replaces: the row loop of get_spectrogram around scipy.signal.spectrogram(row, fs, nperseg, noverlap, nfft, window, scaling)
 * and its average [REF .../spectrograms.py:446-463]: out_power[(nfft / 2 + 1)][nseg], nseg = (frames - noverlap) / (nperseg -
 * noverlap), the mean over the rows of the one-sided power of every segment, each segment detrended by its mean (scipy's
 * default) and multiplied by window[nperseg]; every bin doubled but DC and, for an even nfft, Nyquist.  nfft >= nperseg: the
 * padding is never multiplied.  The rows are added in a fixed order without atomics: the same call returns the same bits.  The
 * cos / sin tables are made on the host in slabs of bins sized against the free device memory; when the means, the result and
 * one slab of 64 bins do not fit beside the 1/16 of the device the context keeps: FSI_ERR_INVALID with both byte counts,
 * nothing allocated, nothing paged, out_power untouched.  The same for nfft > 2^26, the longest table the host is asked for. */
int fsi_spec_spectrogram(FsiCtx* ctx, int32_t quantity, int64_t nperseg, int64_t noverlap, int64_t nfft, const double* window,
                         int32_t scaling, double fs, double* out_power);
/* Replaces: the row loop of get_psd around scipy.signal.periodogram(row, fs, window, scaling) and its average
 * [REF .../spectrograms.py:409-419]: out_power[frames / 2 + 1], the spectrogram of one segment of all recorded frames with nfft =
 * frames (any length, odd included), window[frames]. */
int fsi_spec_periodogram(FsiCtx* ctx, int32_t quantity, const double* window, int32_t scaling, double fs, double* out_power);
/* Replaces: the running total `Pxx_matrix + Pxx` of get_spectrogram's row loop and its division by the row count after the
 * loop [REF .../spectrograms.py:448-463], for a list of total rows that goes through the session in strips: this session holds
 * rows first_row .. first_row + rows - 1 of it.  Arguments as fsi_spec_spectrogram, then: carry[(nfft / 2 + 1)][nseg], the
 * layout of out_power, holds the sum over the row blocks (128 rows each) of the rows before first_row; with first_row == 0
 * its content is ignored and the sum starts from +0.0.  On return it holds that sum with this session's row blocks added, in
 * index order - the additions fsi_spec_spectrogram makes on all rows, so the bits are those of the unsplit call.  total_rows
 * == 0: more strips follow; total_rows > 0: this is the last strip and carry returns the mean over total_rows rows.
 * FSI_ERR_INVALID with one line in fsi_last_error, nothing allocated and carry untouched: first_row < 0 or not a multiple of
 * 128; total_rows == 0 and the session's row count not a multiple of 128 (a later strip's blocks would be cut differently);
 * total_rows != 0 and total_rows != first_row + rows; a null carry; and every refusal of fsi_spec_spectrogram, the room check
 * of the transform included.  No atomics. */
int fsi_spec_spectrogram_sum(FsiCtx* ctx, int32_t quantity, int64_t nperseg, int64_t noverlap, int64_t nfft, const double* window,
                             int32_t scaling, double fs, int64_t first_row, int64_t total_rows, double* carry);
/* Replaces: the running total `Pxx_matrix += Pxx` of get_psd's row loop and its division by the row count
 * [REF .../spectrograms.py:409-417], in strips of rows: fsi_spec_periodogram with the carry of fsi_spec_spectrogram_sum,
 * carry[frames / 2 + 1]; the same checks and refusals. */
int fsi_spec_periodogram_sum(FsiCtx* ctx, int32_t quantity, const double* window, int32_t scaling, double fs, int64_t first_row,
                             int64_t total_rows, double* carry);
/* Replaces: reading rows back from <quantity>_<component>.npz [REF .../spectrograms.py:291-329], for a checkpoint:
 * out[count][rows], frames first .. first + count - 1 of the raw history in one copy.  The rows are what was recorded: with
 * FSI_SPEC_MAG the magnitudes.  Checks and refusals as fsi_band_export. */
int fsi_spec_export(FsiCtx* ctx, int32_t quantity, int64_t first, int64_t count, double* out);
/* Replaces: count calls of fsi_spec_sample after a restart: frames[count][rows] (what fsi_spec_export gave, of a session
 * on the same rows) are appended to the history and, as recording a frame does, the raw series is selected.  Checks and
 * refusals as fsi_band_import. */
int fsi_spec_import(FsiCtx* ctx, int32_t quantity, int64_t count, const double* frames);
/* Closes the session of the quantity and frees its device memory (fsi_destroy does the same). */
int fsi_spec_end(FsiCtx* ctx, int32_t quantity);

/* ---- timing of the device kernels (HIP events on the solver stream) ---------------------------------- */
typedef struct FsiTimers {
  double residual_ms;  int64_t residual_calls;
  double jacobian_ms;  int64_t jacobian_calls;
  double factor_ms;    int64_t factor_calls;
  double spmv_ms;      int64_t spmv_calls;
  double precond_ms;   int64_t precond_calls;
  double ortho_ms;     int64_t ortho_calls;
  double krylov_ms;    int64_t krylov_solves;   int64_t krylov_iters;
  int64_t inner_vv_iters;                    /* fine-level Chebyshev product sweeps LAUNCHED by the block preconditioner (a chain whose  */
                                             /* last sweep is left to its consumer counts one less): velocity block, solid + fluid part  */
  int64_t inner_schur_iters;                 /* ... pressure Schur complement                                          */
  int64_t inner_dd_iters;                    /* ... displacement block                                                 */
  int64_t precond_applies;
  double solid_spmv_ms;  int64_t solid_spmv_calls;   /* sampled launches of the solid-block SpMV (Chebyshev sweeps)   */
  int64_t solid_nnz;     int64_t solid_rows;         /* size of that block                                            */
  double db_spmv_ms;     int64_t db_spmv_calls;      /* sampled launches of the FP32 component-diagonal SpMV          */
  int64_t db_pairs;      int64_t db_nodes;           /* node pairs / nodes of that structure                          */
  double sc_spmv_ms;     int64_t sc_spmv_calls;      /* sampled launches of the scalar-ratio displacement SpMV        */
  int64_t disp_scalar;                               /* bit 0: displacement sweeps use that kernel; bit 1: LDS-tiled  */
  int64_t tile_entries;                              /* total length of the per-tile distinct-neighbour lists         */
  /* orthogonalisation of the recycled GCR: columns of Q / of the direction store streamed since the last reset, and the
     number of launches that streamed them (bytes = columns x ld x element size; see csrc/fsi_gcr.hip)                 */
  int64_t ortho_q_cols;  int64_t ortho_q_launches;
  int64_t ortho_z_cols;  int64_t ortho_z_launches;
  int64_t q_elem_bytes;                              /* 4: Q stored in FP32, 8: FP64                                   */
  int64_t ldq;           int64_t ldz;                /* column strides of Q and of the direction store (elements)     */
  int64_t krylov_dirs;   int64_t krylov_cap;         /* directions currently kept / capacity                          */
  int64_t schur_nnz;     int64_t schur_rows;         /* explicit Schur complement                                     */
  double flush_ms;       int64_t flush_calls;        /* k_gcr_flush (one pass over the direction store per solve)     */
  double schur_ms;       int64_t schur_calls;        /* sampled launches of the Schur-complement sweep                */
  int64_t schur_elem_bytes;                          /* value bytes next to a 4-byte column: 8 FP64, 4 FP32; 0: FP16
                                                        value and 16-bit tile-local column packed in the 4 bytes     */
  int64_t node_pairs;    int64_t node_vertex_pairs;  /* P2 node pairs / node-vertex pairs of the matrix graph         */
  int64_t spmv_fp32_calls;                           /* outer products that ran on the FP32 copy of the matrix        */
  int64_t sweep_flags;                               /* what the preconditioner sweeps actually run as (the context's
                                                        state, not the environment's): bit 0 tiled sweeps fused with
                                                        the Chebyshev update, 1 FP16 packed records, 2 solid block in
                                                        FP32, 3 solid sweeps fused (block Jacobi), 4 solid two-level
                                                        cycle ready, 5 displacement two-level cycle ready, 6 the
                                                        outer products take the displacement rows from their pair
                                                        form (FsiTuning.compact_drows, checked at the last refresh)   */
  int64_t part_allreduces;                           /* partitioned runs: all-reduces issued inside Krylov iterations
                                                        (FP64 basis: one per Gram-Schmidt pass; FP32 basis: two per pass
                                                        + one for its FP64 window; + one when an iteration looks
                                                        converged)                                                    */
  int64_t assembly_colours;                          /* colours of the assembly colouring (one launch of the residual /
                                                        Jacobian kernel each: bitwise reproducible scatter-adds); 0: one
                                                        launch over all cells with unordered atomics (FSI_ASSEMBLY=atomic) */
  /* what the linear solver had to do beyond iterating                                      */
  int64_t gcr_arnoldi_steps;                         /* directions made from the last q because the residual had not moved   */
  int64_t gcr_restarts;                              /* solves that dropped the kept directions (pairs lost / full store stalled) */
  int64_t newton_retries;                            /* Newton iterations whose solve failed on a stale Jacobian and succeeded
                                                        after a refresh                                                      */
  int64_t fp32_fallbacks;                            /* Jacobian lifetimes that lost the FP32 basis and finished in FP64      */
  int64_t verdicts_skipped;                          /* FP32 basis: loose answers (>= 1e-3) returned on the recurrence residual */
  int64_t reorth_forced;                             /* second Gram-Schmidt passes made because the first one showed the kept
                                                        columns non-orthonormal                                              */
  int64_t dd_cache_hits;                             /* Jacobian refreshes that found the displacement block unchanged (three
                                                        checksums) and kept its coarse operator and eigenvalue estimate      */
  int64_t newton_late_solves;                        /* Newton iterations solved with the late (tighter) forcing term        */
} FsiTimers;
/* ---- the solid cycle's exact coarse solve (round 5, csrc/fsi_bcr.hip): test and planning hooks ---------------------------- */
/* Host-only dry run of the planner on any symmetric vertex graph (no device): stats_out[8] = usable, blocks (BFS levels), largest
 * block [unknowns], reduction levels, operator bytes (FP32), set-up arena bytes (FP64), set-up flops, launches per solve; pos_out /
 * level_out (may be NULL): [nc] position in BFS-level order / BFS level of every node. */
int fsi_bcr_plan_graph(int64_t nc, const int64_t* cptr, const int32_t* ccol, int64_t* stats_out, int32_t* pos_out, int32_t* level_out);
/* out[12]: coarse nodes, 3x3 blocks, planned, ready (operators of the current Jacobian), BFS blocks, reduction levels, operator
 * bytes, launches per solve, largest block, solves so far, set-up flops per refresh, two-level cycle ready */
int fsi_solid_coarse_info(const FsiCtx* ctx, int64_t* out);
/* the coarse level's block-CSR operator as the sweeps / the reduction see it: cptr[nc + 1], ccol[nblk], cvals[9 nblk] */
int fsi_solid_coarse_matrix(FsiCtx* ctx, int64_t* cptr, int32_t* ccol, float* cvals);
/* x = A_c^-1 rhs by the production kernels (3 doubles per coarse node) */
int fsi_solid_coarse_solve(FsiCtx* ctx, const double* rhs, double* x);

/* Host-only test hook of the XCD-aware workgroup order (csrc/fsi_kernels.hpp: xcd_unit / xcd_span) that k_residual and the sweep
 * kernels use: unit_out[span] = the unit (tile, cell pair, row block) logical workgroup L of a launch over n units works on, -1 for
 * a workgroup without one; returns span = the number of logical workgroups launched (unit_out may be NULL), -1 for n < 0. */
int64_t fsi_xcd_order(int64_t n, int64_t* unit_out);

int fsi_get_timers(FsiCtx* ctx, FsiTimers* out, int reset);
/* Run totals since fsi_create, without resolving the phase timers (no device synchronisation, safe to call every time step,
 * unaffected by fsi_get_timers(reset = 1)): out[0] newton_retries, out[1] fp32_fallbacks, out[2] gcr_restarts - what the product
 * driver prints as "Linear solver events so far" (the FsiTimers fields of the same names count since the last reset) -, out[3]
 * Newton solves whose tolerance came from the adaptive forcing term, out[4] times such a solve was tightened because its UNSCALED
 * residual was above the tolerance, out[5] exact coarse solves of the solid cycle, out[6], out[7] reserved (0). */
int fsi_get_solver_events(const FsiCtx* ctx, int64_t out[8]);
/* Measurement aid: streams `bytes` of the (idle) Krylov store once per kernel with 4-, 8-, 16- and 32-byte loads and
 * 4-, 8-, 16-byte stores per lane (kernels k_cal_read<...> / k_cal_write<...>), so that a rocprofv3 --pmc FETCH_SIZE /
 * WRITE_SIZE pass can be calibrated against known byte counts at the access widths the solver kernels use.  Discards
 * the recycled Krylov directions. */
int fsi_calibration_streams(FsiCtx* ctx, int64_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* VASPFSI_H */
