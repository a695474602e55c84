/* tinympc_hip.h -- C ABI of libtinympc_hip.so: the MI355X (gfx950) implementation of TinyMPC's
 * ADMM hot path behind the reference's MEX verb surface.
 *
 * The reference exposes ONE MEX function, tinympc_matlab('<verb>', args...), dispatching 17 string
 * verbs onto a process-global solver (/root/reference/src/bindings.cpp:17, 641-692). This header
 * declares one extern "C" function per verb, taking an explicit handle instead of the global, raw
 * column-major `const double*` buffers with explicit sizes instead of mxArrays, and returning an
 * int status instead of long-jumping out through mexErrMsgIdAndTxt. A MEX shim that forwards the
 * 17 verbs to these functions is in tinympc-matlab_amd/matlab/tinympc_matlab_mex.cpp; INTEGRATION.md
 * shows the binding a maintainer would add.
 *
 * Conventions
 *  - All matrices are FP64, column-major, column = knot point (reference types.hpp:15-17,
 *    bindings.cpp:40-41). Inputs are copied during the call (the caller keeps ownership);
 *    outputs are written into caller-allocated buffers.
 *  - Every function returns TINYMPC_OK (0) or a negative TINYMPC_ERR_* code; the message is
 *    available from tinympc_last_error() (thread-local). Nothing throws or long-jumps.
 *  - Threading: a handle is externally synchronised -- one caller at a time per handle; DIFFERENT handles may be driven
 *    from different threads concurrently (one handle per thread, or one per GPU, is the intended use). The library keeps
 *    no other shared mutable state than (a) the run-time specialiser's kernel cache and (b) the registry of open closed-loop
 *    sessions, both behind their own mutexes. The one place where a call reaches into a handle it was not given --
 *    tinympc_setup / tinympc_setup_batch / tinympc_reset sending the resident session kernels of OTHER handles on the same
 *    device home before they allocate or free device memory -- takes that handle's session mutex, which
 *    tinympc_session_step holds for the duration of a tick: a tick in flight on another thread completes undisturbed, and
 *    its handle cannot be destroyed under the walk (it leaves the registry first).
 *  - A handle owns one HIP stream and all its device buffers, and is bound to one GPU. tinympc_solve is synchronous.
 *  - There is NO CPU fallback: without a GPU / without the gfx950 code object every compute verb
 *    fails with TINYMPC_ERR_NO_DEVICE or TINYMPC_ERR_HIP.
 */
#ifndef TINYMPC_HIP_H
#define TINYMPC_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define TINYMPC_ABI_VERSION 1

#define TINYMPC_OK 0
#define TINYMPC_ERR_INVALID_INPUT (-1)   /* MEX id TinyMPC:InvalidInput   (bindings.cpp:22,50,...) */
#define TINYMPC_ERR_NOT_INITIALIZED (-2) /* MEX id TinyMPC:NotInitialized (bindings.cpp:113,...)   */
#define TINYMPC_ERR_HIP (-3)             /* a HIP runtime call failed (message has the hipError)   */
#define TINYMPC_ERR_UNSUPPORTED (-4)     /* problem shape outside what the kernels support         */
#define TINYMPC_ERR_NOT_IMPLEMENTED (-5) /* reserved: no verb returns it any more (every verb is implemented) */
#define TINYMPC_ERR_NO_DEVICE (-6)       /* no HIP device visible                                  */
#define TINYMPC_ERR_ALLOC (-7)

/* solver status values, as the reference core reports them (admm.cpp:114, 183) */
#define TINYMPC_STATUS_SOLVED 1
#define TINYMPC_STATUS_UNSOLVED 11

typedef struct tinympc_solver tinympc_solver; /* opaque */

const char *tinympc_last_error(void);
int tinympc_abi_version(void);
/* Number of visible HIP devices (0 when none); never fails. */
int tinympc_device_count(void);

/* ---------------------------------------------------------------------------------------------
 * The 17 MEX verbs (bindings.cpp:641-692). `verbose` is the trailing scalar every verb takes.
 * ------------------------------------------------------------------------------------------- */

/* verb 'setup'  (bindings.cpp:47-104 -> tiny_setup, tiny_api.cpp:21-122).
 * A nx*nx, B nx*nu, fdyn nx (may be NULL = zeros), Q nx*nx, R nu*nu (only the diagonals of Q and R
 * are used, tiny_api.cpp:90-91). Allocates the handle, uploads the problem, runs the LQR-cache
 * precompute kernel (tiny_precompute_and_set_cache, tiny_api.cpp:124-190) on the device and installs
 * the core's default settings (tiny_api.cpp:213-231). Equivalent to
 * tinympc_setup_batch(out, ..., batch=1, device=-1). */
int tinympc_setup(tinympc_solver **out, const double *A, const double *B, const double *fdyn,
                  const double *Q, const double *R, double rho, int nx, int nu, int N, int verbose);

/* verb 'set_x0' (bindings.cpp:107-131 -> tiny_set_x0, tiny_api.cpp:233-243). len must be nx.
 * In a batched handle this sets instance 0. */
int tinympc_set_x0(tinympc_solver *s, const double *x0, int len, int verbose);

/* verb 'set_x_ref' (bindings.cpp:134-158 -> tiny_api.cpp:245-255). Xref is nx x N. */
int tinympc_set_x_ref(tinympc_solver *s, const double *Xref, int rows, int cols, int verbose);

/* verb 'set_u_ref' (bindings.cpp:161-185 -> tiny_api.cpp:257-267). Uref is nu x (N-1). */
int tinympc_set_u_ref(tinympc_solver *s, const double *Uref, int rows, int cols, int verbose);

/* verb 'set_bound_constraints' (bindings.cpp:188-209). x_min/x_max nx x N, u_min/u_max nu x (N-1),
 * already expanded by the caller (TinyMPC.m:256-264). Enables both bound flags (bindings.cpp:206-207). */
int tinympc_set_bound_constraints(tinympc_solver *s, const double *x_min, const double *x_max,
                                  const double *u_min, const double *u_max, int verbose);

/* verb 'solve' (bindings.cpp:212-232 -> tiny_solve -> solve(), admm.cpp:109-207). One kernel launch
 * runs the whole ADMM loop, in-kernel termination included, for every instance of the handle.
 * Returns TINYMPC_OK whether or not the solver converged (the MEX verb swallows the core status,
 * bindings.cpp:224-231); the core status is reported by tinympc_get_stats. */
int tinympc_solve(tinympc_solver *s, int verbose);

/* verb 'get_solution' (bindings.cpp:235-261): x_out nx*N, u_out nu*(N-1) = the projected slack
 * variables vnew/znew (admm.cpp:187-188, 204-205). Instance 0 of a batched handle. */
int tinympc_get_solution(tinympc_solver *s, double *x_out, double *u_out, int verbose);

/* verb 'get_stats' (bindings.cpp:264-285): iter, status, primal_residual_state, primal_residual_input. */
int tinympc_get_stats(tinympc_solver *s, int *iter, int *status, double *pri_res_state,
                      double *pri_res_input, int verbose);

/* verb 'codegen' (bindings.cpp:288-316 -> tiny_codegen, codegen.cpp:56-68): writes
 * <output_dir>/tinympc/tiny_data.hpp, <output_dir>/src/tiny_data.cpp and <output_dir>/src/tiny_main.cpp from
 * the cache on the device, the settings, the dynamics and the bounds. Copying the solver sources next to them
 * is the caller's job, as in the reference (TinyMPC.m:415-434). */
int tinympc_codegen(tinympc_solver *s, const char *output_dir, int verbose);

/* Everything the emitter writes, as plain host pointers (column-major). tinympc_codegen() fills this from a
 * handle; tinympc_codegen_emit() is host-only file writing and needs no device. */
typedef struct tinympc_codegen_data {
    int nx, nu, N;
    int iter, solved;                                              /* TinySolution.iter / .solved at the time of the call */
    double rho;
    const double *Kinf, *Pinf, *Quu_inv, *AmBKt;                   /* nu x nx, nx x nx, nu x nu, nx x nx */
    const double *dKinf_drho, *dPinf_drho, *dC1_drho, *dC2_drho;   /* emitted only when adaptive_rho != 0; may be NULL */
    double abs_pri_tol, abs_dua_tol;
    int max_iter, check_termination, en_state_bound, en_input_bound, adaptive_rho;
    const double *Q, *R;                                           /* cost diagonals INCLUDING rho: nx, nu (tiny_api.cpp:90-91) */
    const double *Adyn, *Bdyn;                                     /* nx x nx, nx x nu */
    const double *x_min, *x_max, *u_min, *u_max;                   /* nx x N, nx x N, nu x (N-1), nu x (N-1) */
} tinympc_codegen_data;
int tinympc_codegen_emit(const tinympc_codegen_data *data, const char *output_dir, int verbose);

/* verb 'set_sensitivity_matrices' (bindings.cpp:319-361; there it only prints the norms). dK (nu x nx) and
 * dP (nx x nx) become the cache's dKinf_drho / dPinf_drho that the adaptive-rho update reads
 * (rho_benchmark.cpp:205-206); dC1 / dC2 are validated and otherwise unused (they would update the copies
 * C1 / C2, which no solve phase reads). Zero until set. */
int tinympc_set_sensitivity_matrices(tinympc_solver *s, const double *dK, const double *dP,
                                     const double *dC1, const double *dC2, int verbose);

/* verb 'set_cache_terms' (bindings.cpp:364-405): overwrite Kinf (nu x nx), Pinf (nx x nx),
 * Quu_inv (nu x nu), AmBKt (nx x nx); C1/C2 alias the last two. */
int tinympc_set_cache_terms(tinympc_solver *s, const double *Kinf, const double *Pinf,
                            const double *Quu_inv, const double *AmBKt, int verbose);

/* verb 'set_linear_constraints' (bindings.cpp:408-431): rows of Alin_x (nlx x nx) * x <= blin_x and
 * Alin_u (nlu x nu) * u <= blin_u at every knot; a non-empty side is auto-enabled (:422-429).
 * PARITY UNPINNED (no core source in the reference tree). */
int tinympc_set_linear_constraints(tinympc_solver *s, const double *Alin_x, const double *blin_x,
                                   int nlx, const double *Alin_u, const double *blin_u, int nlu);

/* verb 'set_cone_constraints' (bindings.cpp:433-478): per cone (start row Ac, 0-based; dimension qc;
 * slope c), constraint ||s[Ac : Ac+qc-1)||_2 <= c * s[Ac+qc-1] at every knot. State cones first,
 * then input cones (the MATLAB-side order). PARITY UNPINNED. */
int tinympc_set_cone_constraints(tinympc_solver *s, const int *Acx, const int *qcx, const double *cx,
                                 int ncx, const int *Acu, const int *qcu, const double *cu, int ncu);

/* verb 'codegen_with_sensitivity' (bindings.cpp:481-529 -> codegen.cpp:70-90): as 'codegen'; the four
 * sensitivity matrices are written into the generated cache only while adaptive_rho is enabled. */
int tinympc_codegen_with_sensitivity(tinympc_solver *s, const char *output_dir, const double *dK,
                                     const double *dP, const double *dC1, const double *dC2,
                                     int verbose);

/* verb 'reset' (bindings.cpp:532-545): destroy the handle and free every host and device buffer.
 * *s is set to NULL. Passing NULL / a NULL handle is a no-op, as in the reference. */
int tinympc_reset(tinympc_solver **s, int verbose);

/* verb 'update_settings' (bindings.cpp:548-603), same argument order as the MEX verb. With
 * adaptive_rho != 0 solve runs the adaptive-rho loop of the old core (admm.cpp:117-174, rho_benchmark.cpp) on
 * the device, per instance; it cannot be combined with the cone / linear families (TINYMPC_ERR_UNSUPPORTED
 * at solve). */
int tinympc_update_settings(tinympc_solver *s, double abs_pri_tol, double abs_dua_tol, int max_iter,
                            int check_termination, int en_state_bound, int en_input_bound,
                            int en_state_soc, int en_input_soc, int en_state_linear,
                            int en_input_linear, int adaptive_rho, double adaptive_rho_min,
                            double adaptive_rho_max, int adaptive_rho_enable_clipping, int verbose);

/* verb 'print_problem_data' (bindings.cpp:606-638): prints the same scalars to stdout. */
int tinympc_print_problem_data(tinympc_solver *s);

/* ---------------------------------------------------------------------------------------------
 * Methods the reference implements in MATLAB inside the class (no MEX verb); here they run on the
 * device and the .m class / Python mirror forward to them. Any output pointer may be NULL.
 * ------------------------------------------------------------------------------------------- */

/* TinyMPC.compute_cache_terms (src/TinyMPC.m:194-221): Riccati recursion on the FULL user Q, R with rho
 * added once, P0 = Q, gain solve regularised by 1e-8, at most 5000 steps, stop at ||K - Kprev||_2 < 1e-10.
 * Outputs Kinf (nu x nx), Pinf (nx x nx), Quu_inv (nu x nu), AmBKt (nx x nx), column-major. */
int tinympc_compute_cache_terms(tinympc_solver *s, double *Kinf, double *Pinf, double *Quu_inv,
                                double *AmBKt, int *riccati_iters, int verbose);

/* TinyMPC.solve_lqr (src/TinyMPC.m:336-366): stabilising DARE solution for Q + rho_val*I, R + rho_val*I
 * (MATLAB calls idare; here the recursion runs until K is stationary to rounding). C1 = inv(R_rho + B'PB),
 * C2 = (A - BK)'. */
int tinympc_solve_lqr(tinympc_solver *s, double rho_val, double *K, double *P, double *C1, double *C2,
                      int *riccati_iters);

/* TinyMPC.compute_sensitivity_autograd (src/TinyMPC.m:223-241): forward differences of solve_lqr in rho
 * with h = 1e-6. dK (nu x nx), dP (nx x nx), dC1 (nu x nu), dC2 (nx x nx). */
int tinympc_compute_sensitivity(tinympc_solver *s, double *dK, double *dP, double *dC1, double *dC2,
                                int verbose);

/* ---------------------------------------------------------------------------------------------
 * Extensions (not in the reference): cache read-back, batched mode, timing.
 * ------------------------------------------------------------------------------------------- */

/* Read back what the precompute kernel produced (any pointer may be NULL). riccati_iters = number
 * of fixed-point steps taken before max|dK| < 1e-5 (tiny_api.cpp:157). */
int tinympc_get_cache(tinympc_solver *s, double *Kinf, double *Pinf, double *Quu_inv, double *AmBKt,
                      int *riccati_iters);

/* All four residuals of instance 0: primal state, dual state, primal input, dual input
 * (admm.cpp:93-96). */
int tinympc_get_residuals(tinympc_solver *s, double residuals[4]);

/* Batched setup: `batch` independent MPC instances sharing (A,B,fdyn,Q,R,rho,settings) and, by default, bounds and refs,
 * each with its own x0 and its own persistent ADMM state (references per instance: tinympc_set_x_ref_batch below; bounds per
 * instance: tinympc_set_bound_constraints_batch below; models per instance: tinympc_set_model_batch below). device < 0 keeps the current HIP device. */
int tinympc_setup_batch(tinympc_solver **out, const double *A, const double *B, const double *fdyn,
                        const double *Q, const double *R, double rho, int nx, int nu, int N,
                        int batch, int device, int verbose);

/* x0s is nx x count (column b = instance first+b), host memory. Single-instance handles: the same as tinympc_set_x0 for launched
 * AND resident solves (both forms also bring the pinned copy up to date that a resident solve hands to its session), except that
 * they need the device and so end an open session. */
int tinympc_set_x0_batch(tinympc_solver *s, const double *x0s, int first, int count);
/* Same, from device memory on the handle's GPU (e.g. a torch tensor's data_ptr). Contract: whatever
 * PRODUCED d_x0s on another stream must have completed before the call (the copy runs on the handle's own
 * non-blocking stream, which is ordered against no other stream); the copy itself has completed when the
 * call returns, so the caller may free or overwrite d_x0s right away. */
int tinympc_set_x0_batch_device(tinympc_solver *s, const double *d_x0s, int first, int count);

/* Per-instance references for instances [first, first+count) of a batched handle.
 * Xrefs: nx x cols x count, column-major, instance b's block at b*nx*cols; cols = N (a trajectory per instance)
 *        or cols = 1 (one goal per instance, held over the whole horizon). Urefs likewise with nu and N-1.
 * Instance b then solves exactly what it would solve alone after set_x_ref(Xref_b) / set_u_ref(Uref_b). The first call
 * for a half (x or u) turns per-instance mode on for that half; instances outside the range keep the handle's shared
 * reference of that moment. A later tinympc_set_x_ref / tinympc_set_u_ref returns that half to shared mode for every
 * instance. reset_workspace, update_settings, set_bound_constraints, the solve verbs and mpc_step_batch keep them.
 * Goals run on layout D where the handle runs layout D (compiled in or run-time specialised) -- and, 16-lane shapes with a batch
 * beyond one resident set and tolerances that can be met, with slot refill (tinympc_get_jit_info: " goal slot-refill"; bit-identical
 * results; TINYMPC_REFILL as for the shared reference; the trajectory form of layout D, below, refills in the same way beyond ITS
 * resident set: " per-instance-trajectories slot-refill"). Trajectories (either half, cols = N /
 * N-1) run on layout A -- or, on a handle that called tinympc_prepare (before or after these verbs), on layout D's per-instance
 * trajectory form: where the handle runs layout D with nx+nu <= 16, bounds are constant over the horizon (shared or per instance), the
 * model and rho are the shared ones, and the horizon's N+2 reference rows fit a wavefront's share of LDS beside its other state (the
 * plan's arithmetic decides; for the quadrotor, nu = 4, that is a horizon of about 60 -- N = 50 is compiled in, other shapes are
 * specialised at run time). With bounds that vary over the horizon -- per instance (tinympc_set_bound_constraints_batch with cols = N)
 * or shared -- the form also holds the wavefront's 2 (N+2) clamp rows (" per-knot-bounds" beside " per-instance-trajectories"; box
 * path only; quadrotor: N <= 22, N = 20 compiled in; " per-knot-bounds(no plan)" and layout A beyond). Whatever misses a condition
 * stays on layout A; tinympc_get_layout and tinympc_get_jit_info
 * (" per-instance-trajectories", or "refused(...)" with the reason) say which ran. Inside the per-instance families mode
 * (tinympc_set_linear_constraints_batch, _knots_batch, tinympc_set_cone_slopes_batch) trajectories sent through THESE verbs keep a
 * prepared handle on layout D as well (see there); a trajectory shared by the batch that arrives through tinympc_set_x_ref /
 * tinympc_set_u_ref moves that mode to layout A -- a caller who wants layout D sends it through the batch verb.
 * With the cone / linear families, adaptive rho or nx+nu > 64 a solve returns TINYMPC_ERR_UNSUPPORTED (never a solve with
 * the shared reference). The _device forms refuse memory that is not device memory of the handle's GPU.
 * Single-instance handles: the same as tinympc_set_x_ref / tinympc_set_u_ref. The input has been copied when the call
 * returns. */
int tinympc_set_x_ref_batch(tinympc_solver *s, const double *Xrefs, int rows, int cols, int first, int count);
int tinympc_set_u_ref_batch(tinympc_solver *s, const double *Urefs, int rows, int cols, int first, int count);
/* Same, from device memory on the handle's GPU; same contract as tinympc_set_x0_batch_device. */
int tinympc_set_x_ref_batch_device(tinympc_solver *s, const double *d_Xrefs, int rows, int cols, int first, int count);
int tinympc_set_u_ref_batch_device(tinympc_solver *s, const double *d_Urefs, int rows, int cols, int first, int count);

/* Reference tracks: per-instance sliding reference windows kept on the device ("upload once, step per tick").
 * Xtracks: nx x T x count, column-major, instance b's block at b*nx*T; Utracks: nu x T x count likewise. T >= 1 is the track's length
 * in knots, independent of N and of the other half's. Every instance also has a step k >= 0 (one per instance, serving both halves;
 * 0 until set). Instance b at step k then solves exactly what it would solve after tinympc_set_x_ref_batch with the trajectory
 * X_b[:, min(k+i, Tx-1)], i = 0..N-1, and tinympc_set_u_ref_batch with U_b[:, min(k+i, Tu-1)], i = 0..N-2 -- bit for bit, on the same
 * kernel: the last knot is held beyond the end of the track, and the window's rows are built on the device from track and step by
 * the row builder of the per-instance references (from the instance's own Pinf and cost diagonals when per-instance models are on), so
 * a closed-loop tick uploads x0 and nothing else.
 * Track mode is per half. The first track call of a half must name the whole batch (first = 0, count = batch); later calls may
 * replace a sub-range with the same T, a whole-batch call may change T; replacing a track does not touch the steps. A half in track
 * mode IS a half with per-instance trajectories: it turns per-instance references on for that half, runs on layout A (even with
 * T = 1: never layout D's goal form) -- or, after tinympc_prepare and under tinympc_set_x_ref_batch's conditions, on layout D's
 * per-instance trajectory form (with bounds per knot: on its per-knot bounds form, see there), or, inside the per-instance families mode, on that mode's form for trajectories
 * (tinympc_set_linear_constraints_batch; tinympc_mpc_step_batch with auto-advance included: the rows are rebuilt per tick as on layout A,
 * and the kernel stages the rebuilt rows; the trajectory and per-knot bounds forms run a tick beyond one resident set with slot refill,
 * see tinympc_get_jit_info) --,
 * " reference-track" is appended to tinympc_get_jit_info, and every refusal of per-instance
 * references applies unchanged (the cone / linear families, adaptive rho, nx+nu > 64: a solve returns TINYMPC_ERR_UNSUPPORTED;
 * tinympc_session_begin likewise). tinympc_set_x_ref / _u_ref returns the half to shared references; a whole-batch
 * tinympc_set_x_ref_batch / _u_ref_batch returns it to plain per-instance references, while one on a sub-range returns
 * TINYMPC_ERR_INVALID_INPUT (name the whole batch). The store of a half that left the mode is kept for its next track; the steps stay.
 * reset_workspace, update_settings, the bound and model verbs, the solve verbs and mpc_step_batch keep tracks and steps.
 * Everything is validated before anything is written: invalid arguments (a first call on a sub-range, a sub-range call with another
 * T, T < 1, a range beyond the batch, a negative step, host memory or another GPU's memory handed to a _device form) return
 * TINYMPC_ERR_INVALID_INPUT and leave mode, store, steps and rows as they were, and so does a failed allocation (TINYMPC_ERR_ALLOC).
 * Single-instance handles: the same verbs on instance 0 -- the library keeps the track on the host and forwards the current window
 * through tinympc_set_x_ref / tinympc_set_u_ref whenever track or step changes, so the families, the session and resident solves work
 * with tracks (inside a session a window moved up by one knot sends one column). The input has been copied when the call returns. */
int tinympc_set_x_ref_track_batch(tinympc_solver *s, const double *Xtracks, int rows, int T, int first, int count);
int tinympc_set_u_ref_track_batch(tinympc_solver *s, const double *Utracks, int rows, int T, int first, int count);
/* Same, from device memory on the handle's GPU; same contract as tinympc_set_x0_batch_device. */
int tinympc_set_x_ref_track_batch_device(tinympc_solver *s, const double *d_Xtracks, int rows, int T, int first, int count);
int tinympc_set_u_ref_track_batch_device(tinympc_solver *s, const double *d_Utracks, int rows, int T, int first, int count);
/* The steps of instances [first, first+count): steps[count], each >= 0 (a step beyond the end of a track holds its last knot). The
 * _device form reads device memory of the handle's GPU and validates it there (one flag read back). The rows of the range are
 * rebuilt at the next launch. */
int tinympc_set_ref_step_batch(tinympc_solver *s, const int *steps, int first, int count);
int tinympc_set_ref_step_batch_device(tinympc_solver *s, const int *d_steps, int first, int count);
/* Every instance's step += delta, on the device: one small kernel on the handle's stream, saturating at INT_MAX (it cannot wrap), no
 * copy and no synchronisation for delta >= 0. A delta < 0 that would take some step below 0 returns TINYMPC_ERR_INVALID_INPUT and
 * changes nothing (validated on the device first: one flag read back, for negative deltas only). */
int tinympc_advance_ref_step_batch(tinympc_solver *s, int delta);
/* tinympc_mpc_step_batch adds delta >= 0 to every instance's step AFTER its solve (the tick solves the window of the step it found);
 * nothing is read back. 0 (the default) switches it off. tinympc_mpc_step_batch only: the other solve verbs and the session leave the
 * steps alone. The setting, like the steps, outlives the tracks: while it is on, every tick queues the one small kernel that moves
 * the steps, also on a handle whose halves have both left track mode -- switch it off with the tracks where that launch matters. */
int tinympc_set_ref_auto_advance(tinympc_solver *s, int delta);
int tinympc_get_ref_step_batch(tinympc_solver *s, int *steps_out, int first, int count);

/* Per-instance box bounds for instances [first, first+count) of a batched handle.
 * x_min, x_max: nx x cols x count, column-major, instance b's block at b*nx*cols; u_min, u_max: nu x ucols x count likewise.
 * cols = N (bounds per knot; then ucols = N-1) or cols = 1 (one box per instance, held over the whole horizon; then ucols = 1).
 * Instance b then solves exactly what it would solve alone after set_bound_constraints(bounds_b); like that verb, the call enables
 * both bound families (a later tinympc_update_settings can switch either off again, for every instance). The first call turns
 * per-instance mode on; instances outside the range keep the handle's shared bounds of that moment. A later
 * tinympc_set_bound_constraints returns every instance to shared bounds. reset_workspace, update_settings, the reference verbs, the
 * solve verbs and mpc_step_batch keep them. Boxes (with references constant over the horizon) run on layout D where the handle runs
 * layout D, with slot refill where a shared box would have it (see tinympc_get_jit_info). Bounds per knot run on layout A -- or, on a handle that called tinympc_prepare and runs layout D with nx+nu <= 16, on layout
 * D's per-knot bounds form: box path, the shared model and rho, every reference half constant over the horizon (shared or per instance)
 * or a per-instance trajectory / track, and a horizon whose 2 (N+2) clamp rows (3 (N+2) rows beside trajectories) fit a wavefront's
 * LDS share (quadrotor: N <= 33, N <= 22 beside trajectories; tinympc_get_jit_info says " per-knot-bounds", or " per-knot-bounds(no
 * plan)" where the horizon does not fit; beyond one resident set of that form and with tolerances that can be met it runs with slot
 * refill, " per-knot-bounds slot-refill", bit-identical). What stays on layout A with bounds per knot: no tinympc_prepare, a trajectory shared by the
 * batch through tinympc_set_x_ref / _set_u_ref, per-instance models or rho, per-instance linear rows or cone slopes, wider systems,
 * longer horizons. With the cone / linear families, adaptive rho or nx+nu > 64 a solve returns
 * TINYMPC_ERR_UNSUPPORTED (never a solve with the shared bounds). Invalid arguments return TINYMPC_ERR_INVALID_INPUT and leave the mode
 * as it was. Single-instance handles: the same as tinympc_set_bound_constraints. The input has been copied when the call returns. */
int tinympc_set_bound_constraints_batch(tinympc_solver *s, const double *x_min, const double *x_max,
                                        const double *u_min, const double *u_max, int cols, int first, int count);
/* Same, from device memory on the handle's GPU; same contract as tinympc_set_x0_batch_device. */
int tinympc_set_bound_constraints_batch_device(tinympc_solver *s, const double *d_x_min, const double *d_x_max,
                                               const double *d_u_min, const double *d_u_max, int cols, int first, int count);

/* Per-instance linear (half-space) constraints for instances [first, first+count) of a batched handle: a_k' x <= b_k, a_k' u <= b_k.
 * Alin_x: nlx x nx x count, column-major, instance b's block at b*nlx*nx; blin_x: nlx x count; Alin_u: nlu x nu x count, blin_u:
 * nlu x count likewise. Instance first+b then solves exactly what a single-instance handle would solve after
 * tinympc_set_linear_constraints(Alin_x_b, blin_x_b, nlx, Alin_u_b, blin_u_b, nlu) -- an instance whose rows are the shared ones, bit
 * for bit what the shared rows give on layout A. The row COUNTS (nlx, nlu) belong to the batch, the values to the instance: b = +inf
 * switches one row off for one instance. The first call turns per-instance mode on. It may name a sub-range if the handle holds shared
 * rows of the same (nlx, nlu) at that moment -- the other instances keep those rows --; otherwise it must name the whole batch (first = 0,
 * count = batch). A later call on a sub-range must use the mode's counts; a whole-batch call may change them. At most 32 rows per side
 * (TINYMPC_ERR_UNSUPPORTED beyond). Like the shared verb the call enables the linear family of every non-empty side (a later
 * tinympc_update_settings can switch either side off again, for every instance) and keeps the ADMM state, the family's duals
 * included: replacing the rows between two warm-started ticks is the intended use (obstacle half-spaces re-linearised every tick).
 * tinympc_set_linear_constraints returns every instance to shared rows. reset_workspace, update_settings, the reference, track and
 * bound verbs (shared and per instance), set_cone_constraints, the solve verbs and mpc_step_batch keep mode and rows.
 * The mode runs on layout A (tinympc_get_layout 'A', " per-instance-linear" in tinympc_get_jit_info) unless tinympc_prepare was
 * called on the handle (before or after this verb): then batches that run the register-resident throughput kernel (layout D) keep it
 * -- every wavefront holds its four instances' rows -- where nx+nu <= 16, bounds are constant over the horizon (shared or per
 * instance), every half of the references is constant over the horizon (shared or per instance) or holds per-instance trajectories
 * or a track (tinympc_set_x_ref_batch / _u_ref_batch with cols = N / N-1, the track verbs), no two cones share a row and the horizon
 * and row count fit that kernel's plan (N <= 22); the kernel is compiled in for the quadrotor at N = 20 with one row, specialised at
 * run time otherwise. With per-instance trajectories or tracks every wavefront also holds its four instances' N+2 reference rows
 * (tinympc_get_jit_info: "... per-instance-linear per-instance-trajectories"; compiled in for the same quadrotor with one row): the
 * plan then needs 3 max(nlx, nlu) + N + 2 vectors of 64 doubles beside the wavefront's other state (the quadrotor at N = 20: up to 17
 * rows per side where references constant over the horizon leave room for 24). A trajectory SHARED by the batch (tinympc_set_x_ref / _set_u_ref with columns that
 * differ) keeps the mode on layout A: send it through the batch verb to stay on layout D. Per-knot bounds, wider systems,
 * longer horizons and a refused specialisation (tinympc_get_jit_info then reads "refused(<reason>) ... per-instance-linear") stay on
 * layout A, and a handle moves between the two from one launch to the next as its configuration changes; the ADMM state, the family's
 * duals included, is shared, so a warm start carries over. Either way the mode takes cones -- shared, or with every instance's own
 * slopes (tinympc_set_cone_slopes_batch below: the other half of the same mode) --, fdyn, per-instance references
 * (goals, trajectories, tracks) and per-instance bounds (box or per knot)
 * in any combination: its kernels always read the reference and clamp rows per instance. With per-instance models or rho, adaptive
 * rho, nx+nu > 64 or more cones / rounds than the generic kernels hold a solve returns TINYMPC_ERR_UNSUPPORTED (never a solve with
 * shared rows), and so does tinympc_session_begin. Outside the mode, per-instance references or bounds together with a family stay
 * refused. Invalid arguments -- a row of A that is all zero or not finite, a b that is NaN or -inf, a NULL pointer for a non-empty side,
 * negative counts or no row at all, a range that is empty or beyond the batch, a sub-range with other counts, host memory or another
 * GPU's memory handed to the _device form -- return TINYMPC_ERR_INVALID_INPUT and leave mode, rows, enable flags and ADMM state as
 * they were: everything is validated (on the device, one flag read back) before anything is written. Single-instance handles: the same
 * as tinympc_set_linear_constraints, with count 1. The input has been copied when the call returns. */
int tinympc_set_linear_constraints_batch(tinympc_solver *s, const double *Alin_x, const double *blin_x, int nlx,
                                         const double *Alin_u, const double *blin_u, int nlu, int first, int count);
/* Same, from device memory on the handle's GPU (host and device form give the same bits: one builder); same contract as
 * tinympc_set_x0_batch_device. */
int tinympc_set_linear_constraints_batch_device(tinympc_solver *s, const double *d_Alin_x, const double *d_blin_x, int nlx,
                                                const double *d_Alin_u, const double *d_blin_u, int nlu, int first, int count);

/* Per-KNOT linear (half-space) constraints for instances [first, first+count) of a batched handle: a_{k,i}' x_i <= b_{k,i} at knot i,
 * a_{k,i}' u_i <= b_{k,i} likewise -- the rows' values belong to the knot AND the instance (a moving obstacle, a path round an obstacle,
 * a keep-out corridor that varies over the horizon). Column-major, instance first+b's block at b times the block size:
 *   Alin_x: nlx x nx x N x count     blin_x: nlx x N x count     Alin_u: nlu x nu x (N-1) x count     blin_u: nlu x (N-1) x count
 * Instance first+b solves the ADMM problem of the reference algorithm in which the state-linear slack at knot i is the row-after-row
 * projection of x_i + gl_i onto knot i's own rows (knot 0 included, as the reference's slack update includes it), the input-linear slack
 * likewise; everything else is as in the per-instance families' solve. An instance whose rows are equal at every knot gives, bit for
 * bit, what tinympc_set_linear_constraints_batch gives for those rows on layout A. This is the third state of the rows' half of the
 * per-instance families mode (shared rows; rows per instance, constant over the horizon; rows per instance and knot).
 * The row COUNTS (nlx, nlu) belong to the batch, the values to the knot and the instance: b = +inf switches one row off at one knot. At
 * most 32 rows per side (TINYMPC_ERR_UNSUPPORTED beyond). The FIRST call must name the whole batch (first = 0, count = batch); later
 * calls may replace a sub-range with the same counts; a whole-batch call may change the counts. The call enables the linear family of
 * every non-empty side and keeps the ADMM state, the family's duals included: re-sending shifted rows between two warm
 * tinympc_mpc_step_batch ticks is the intended use.
 * Leaving the mode: tinympc_set_linear_constraints returns every instance to shared rows; a whole-batch
 * tinympc_set_linear_constraints_batch returns the half to rows constant over the horizon; a sub-range
 * tinympc_set_linear_constraints_batch while the rows are per knot returns TINYMPC_ERR_INVALID_INPUT ("name the whole batch") and changes
 * nothing. reset_workspace, update_settings, every reference, track and bound verb (shared or per instance), set_cone_constraints,
 * set_cone_slopes_batch, the solve verbs, mpc_step_batch and prepare keep mode and rows; per-instance cone slopes combine with it (the
 * other half of the same mode, the same store).
 * The mode runs on layout A (tinympc_get_layout 'A', " per-knot-linear" in tinympc_get_jit_info in place of " per-instance-linear")
 * unless tinympc_prepare was called on the handle (before or after this verb): then batches that run the register-resident throughput
 * kernel (layout D) keep it under the conditions of tinympc_set_linear_constraints_batch -- nx+nu <= 16, bounds constant over the
 * horizon, references constant over the horizon or per-instance trajectories / tracks, no two cones share a row -- where every
 * wavefront's share of a compute unit's LDS holds its four instances' rows of ALL knots, 3 max(nlx, nlu) N vectors of 64 doubles: one
 * row per side up to N = 22, two up to N = 12, three up to N = 8. The kernel is compiled in for the quadrotor at N = 20 with one row,
 * specialised at run time otherwise. With per-instance trajectories or tracks the wavefront's N+2 reference rows share that space
 * (" per-knot-linear per-instance-trajectories"): one row per side up to N = 17, two up to N = 10, three up to N = 7 for the
 * quadrotor (nu = 4); the quadrotor at N = 20 with one row per knot and trajectories has no plan and stays on layout A. Without
 * tinympc_prepare, with a shared trajectory, per-knot bounds, wider systems, cones in rounds, or after a refused plan
 * (tinympc_get_jit_info then reads "refused(<reason>) ... per-knot-linear") the mode stays on layout A, and a handle moves between the
 * two from one launch to the next as its configuration changes; the ADMM state, the rows' duals included, is shared, so a warm start
 * carries over. On layout D, too, an instance whose rows are equal at every knot gives, bit for bit, what
 * tinympc_set_linear_constraints_batch gives for those rows there. Refusals are
 * those of tinympc_set_linear_constraints_batch: with per-instance models or rho, adaptive rho, nx+nu > 64 or more cones / rounds than
 * the generic kernels hold a solve returns TINYMPC_ERR_UNSUPPORTED (never a solve with other rows), and so does tinympc_session_begin.
 * Single-instance handles (batch == 1): TINYMPC_ERR_UNSUPPORTED -- their kernels read the shared description.
 * Invalid arguments -- a row of A at some knot that is all zero or not finite, a b that is NaN or -inf, NULL for a non-empty side,
 * negative counts or no row at all, a range that is empty or beyond the batch, a first call on a sub-range, a sub-range with other
 * counts, host memory or another GPU's memory handed to the _device form -- return TINYMPC_ERR_INVALID_INPUT and leave mode, rows, enable
 * flags and ADMM state as they were: everything is validated (on the device, one flag read back) before anything is written. A failed
 * allocation returns TINYMPC_ERR_ALLOC and leaves everything as it was: the store holds 3 max(nlx, nlu) N + 4 vectors of 64 doubles per
 * wavefront (8,192 quadrotors at N = 20 with one row: 67 MB). The input has been copied when the call returns. */
int tinympc_set_linear_constraints_knots_batch(tinympc_solver *s, const double *Alin_x, const double *blin_x, int nlx,
                                               const double *Alin_u, const double *blin_u, int nlu, int first, int count);
/* Same, from device memory on the handle's GPU (host and device form give the same bits: one builder); same contract as
 * tinympc_set_x0_batch_device. */
int tinympc_set_linear_constraints_knots_batch_device(tinympc_solver *s, const double *d_Alin_x, const double *d_blin_x, int nlx,
                                                      const double *d_Alin_u, const double *d_blin_u, int nlu, int first, int count);

/* Per-instance cone slopes for instances [first, first+count) of a batched handle. The cone STRUCTURE (Acx, qcx, Acu, qcu) is the one the
 * handle holds from tinympc_set_cone_constraints and belongs to the batch; the slope values belong to the instance. cx: ncx x count,
 * column-major, instance first+b's slopes at b*ncx in the order of the shared cone list; cu: ncu x count likewise. ncx and ncu must
 * equal the structure's counts; a side without cones takes NULL. Instance first+b then solves exactly what a single-instance handle
 * would solve after tinympc_set_cone_constraints(Acx, qcx, cx_b, ncx, Acu, qcu, cu_b, ncu) -- an instance whose slopes are the shared
 * ones, bit for bit what the shared cones give on the same kernel. The first call turns the slopes' half of the per-instance families
 * mode on; it may name any sub-range: the other instances keep the shared slopes of that moment. The call changes no enable flag (the
 * shared verb enabled the sides; tinympc_update_settings may switch a side off for every instance) and keeps the ADMM state, the
 * cones' duals included: re-sending slopes between two warm-started tinympc_mpc_step_batch ticks is an intended use. A later
 * tinympc_set_cone_constraints installs a new structure and returns every instance to shared slopes. reset_workspace,
 * update_settings, every reference, track and bound verb, both linear verbs, the solve verbs, mpc_step_batch and prepare keep the half
 * and its values.
 * Per-instance slopes and per-instance linear rows (tinympc_set_linear_constraints_batch) are two halves of ONE mode, in either order
 * and each alone: the shared tinympc_set_linear_constraints ends the rows' half only, the shared tinympc_set_cone_constraints the
 * slopes' half only, and the mode ends when both are off. Layout A's kernel of the mode always reads rows and slopes per instance:
 * the half that is off holds the shared values for every instance (one absent row on a handle without linear rows); layout D's form
 * is specialised on the row count and on whether the slopes' half is on. So the mode runs where the rows'
 * mode runs -- layout A (" per-instance-cones" in tinympc_get_jit_info, beside " per-instance-linear" when both halves are on), or,
 * after tinympc_prepare, layout D under the conditions stated above, per-instance trajectories and tracks included (the kernel is
 * compiled in for the rocket landing nx=6 nu=3 N=10 with one row and references constant over the horizon, specialised at run time
 * otherwise -- the landing that follows its reference trajectory per instance among them; cones that share rows stay on layout A) -- and is refused where that mode is
 * refused: with per-instance models or rho, adaptive rho, nx+nu > 64 or more cones / rounds than the generic kernels hold a solve
 * returns TINYMPC_ERR_UNSUPPORTED (never a solve with shared slopes), and so does tinympc_session_begin.
 * Invalid arguments -- a slope that is NaN, infinite or <= 0, a count that differs from the structure's, no cones on the handle, NULL
 * for a non-empty side, a range that is empty or beyond the batch, host memory or another GPU's memory handed to the _device form --
 * return TINYMPC_ERR_INVALID_INPUT and leave mode, slopes, flags and ADMM state as they were: everything is validated (on the device,
 * one flag read back) before anything is written. Single-instance handles: the same as tinympc_set_cone_constraints with the held
 * structure, with count 1. The input has been copied when the call returns. */
int tinympc_set_cone_slopes_batch(tinympc_solver *s, const double *cx, int ncx, const double *cu, int ncu, int first, int count);
/* Same, from device memory on the handle's GPU (host and device form give the same bits: one builder); same contract as
 * tinympc_set_x0_batch_device. */
int tinympc_set_cone_slopes_batch_device(tinympc_solver *s, const double *d_cx, int ncx, const double *d_cu, int ncu, int first, int count);

/* Per-instance models for instances [first, first+count) of a batched handle.
 * A: nx*nx*count, B: nx*nu*count, fdyn: nx*count (NULL = zeros), Q: nx*nx*count, R: nu*nu*count; column-major, instance b's block
 * at b*(block size); of Q and R only the diagonals are used, as in tinympc_setup. N and the settings stay the handle's; rho is the
 * handle's unless tinympc_set_rho_batch below gave the instance its own.
 * Instance b then solves exactly what a single-instance handle set up with (A_b, B_b, fdyn_b, Q_b, R_b, rho_b) would solve: its LQR
 * cache is computed on the device by the kernels of tinympc_setup, one wavefront or workgroup per instance in one launch, and is
 * bit-identical to that handle's. The first call turns per-instance mode on; instances outside the range keep the handle's shared
 * model (and cache) of that moment. tinympc_clear_model_batch returns every instance to the shared model. reset_workspace,
 * update_settings, the reference and bound verbs (shared and per-instance), the solve verbs and mpc_step_batch keep the mode. The
 * single-model verbs (get_cache, set_cache_terms, set_sensitivity_matrices, codegen*, compute_cache_terms, solve_lqr,
 * compute_sensitivity, print_problem_data) keep addressing the SHARED model and cache; tinympc_get_cache_batch reads per instance.
 * The mode runs on layout A unless tinympc_prepare was called on the handle (before or after this verb): then batches that run the
 * register-resident throughput kernel (layout D) keep it -- every wavefront holds its four instances' operators -- where nx+nu <= 16,
 * references and bounds are constant over the horizon (shared or per instance) and the horizon fits that kernel's plan; trajectories,
 * per-knot bounds, wider systems, longer horizons and a refused specialisation (tinympc_get_jit_info says why) stay on layout A. With
 * the cone / linear families, adaptive rho or nx+nu > 64 a solve returns TINYMPC_ERR_UNSUPPORTED (never a solve with the shared model), and so does tinympc_session_begin.
 * Invalid arguments (a NULL A, B, Q or R, a range beyond the batch, count < 1, host memory handed to the _device form) return
 * TINYMPC_ERR_INVALID_INPUT and leave the mode as it was. Single-instance handles: the same, on instance 0. The input has been copied
 * when the call returns. */
int tinympc_set_model_batch(tinympc_solver *s, const double *A, const double *B, const double *fdyn,
                            const double *Q, const double *R, int first, int count);
/* Same, from device memory on the handle's GPU; same contract as tinympc_set_x0_batch_device. */
int tinympc_set_model_batch_device(tinympc_solver *s, const double *d_A, const double *d_B, const double *d_fdyn,
                                   const double *d_Q, const double *d_R, int first, int count);
/* Per-instance ADMM penalty for instances [first, first+count) of a batched handle: rho[count], each a finite number > 0.
 * Instance first+b then solves exactly what a single-instance handle set up with (its model, rho[b]) would solve: its LQR cache is
 * computed on the device by the kernels of tinympc_setup and is bit-identical to that handle's (tinympc_get_cache_batch against
 * tinympc_get_cache, riccati_iters included). This IS the per-instance model mode: the first call enters it exactly as
 * tinympc_set_model_batch does -- every instance starts from the shared model, cache, operators and rho of that moment, instances outside
 * the range keep the shared rho -- and everything that mode implies holds (layout A; layout D's model form after tinympc_prepare, in
 * either order; " per-instance-models" in tinympc_get_jit_info; no slot refill, lean sweeps, session or zero-copy tick).
 * tinympc_clear_model_batch returns every instance to the shared model AND the shared rho. The two verbs commute: the handle keeps
 * every instance's raw cost diagonals and forms Q_b + rho_b by one addition, as tinympc_setup does, so rho then model gives the bits of
 * model then rho and of (model_b, rho_b) from scratch. tinympc_get_rho_batch returns the instance's rho while the mode is on and the
 * setup value again after tinympc_clear_model_batch; reset_workspace, update_settings, the reference and bound verbs (shared and per
 * instance), the solve verbs and mpc_step_batch keep the per-instance values. With the cone / linear families, adaptive rho or
 * nx+nu > 64 a solve returns TINYMPC_ERR_UNSUPPORTED (never a solve with the shared rho), and so does tinympc_session_begin. Invalid
 * arguments (a NULL pointer, a range that is empty or beyond the batch, a value that is not finite or <= 0, host memory or another
 * GPU's memory handed to the _device form) return TINYMPC_ERR_INVALID_INPUT and leave the mode, the store and every cache as they were:
 * everything is validated before anything is written. Single-instance handles: the same, on instance 0. The input has been copied when
 * the call returns. */
int tinympc_set_rho_batch(tinympc_solver *s, const double *rho, int first, int count);
/* Same, from device memory on the handle's GPU (validated there); same contract as tinympc_set_x0_batch_device. */
int tinympc_set_rho_batch_device(tinympc_solver *s, const double *d_rho, int first, int count);
/* Every instance back on the shared model and rho that setup installed. */
int tinympc_clear_model_batch(tinympc_solver *s);
/* The LQR cache of instances [first, first+count): Kinf nu*nx*count, Pinf nx*nx*count, Quu_inv nu*nu*count, AmBKt nx*nx*count,
 * riccati_iters[count]; any pointer may be NULL. Without per-instance models: the shared cache, repeated. */
int tinympc_get_cache_batch(tinympc_solver *s, double *Kinf, double *Pinf, double *Quu_inv, double *AmBKt,
                            int *riccati_iters, int first, int count);

/* Zero the persistent ADMM state (cold start) of every instance and put every instance's rho back to
 * the setup value -- with per-instance models on, to the instance's own set value (tinympc_set_rho_batch); x0 is kept. */
int tinympc_reset_workspace(tinympc_solver *s);

/* Adaptive rho (settings adaptive_rho*, admm.cpp:117-174, rho_benchmark.cpp): every instance carries its own
 * rho, adapted every 5th iteration and kept across solves like the reference's cache->rho. Reads it back for
 * instances [first, first+count). Equals the setup rho while adaptive_rho has never been on. While per-instance models are on
 * (tinympc_set_model_batch / tinympc_set_rho_batch): the instance's own rho. */
int tinympc_get_rho_batch(tinympc_solver *s, double *rho_out, int first, int count);

/* Solutions of instances [first, first+count): x_out nx*N*count, u_out nu*(N-1)*count. */
int tinympc_get_solution_batch(tinympc_solver *s, double *x_out, double *u_out, int first, int count);
/* First control of each instance, nu x count: what a closed-loop caller applies. */
int tinympc_get_first_controls_batch(tinympc_solver *s, double *u0_out, int first, int count);
/* iters[count], status[count], residuals 4 x count (any may be NULL). */
int tinympc_get_stats_batch(tinympc_solver *s, int *iters, int *status, double *residuals, int first,
                            int count);
/* Device pointers of the solution buffers (nx*N*batch and nu*(N-1)*batch doubles), valid until
 * tinympc_reset; lets a caller consume results without a D2H copy. The pointers are stable for the handle's lifetime and
 * need not be queried again after tinympc_reset_workspace: once they have been handed out, a reset zeroes the buffers on
 * the handle's stream itself (before, it only marks them zero and lets the next solve overwrite them). Reads must be
 * ordered behind the handle's stream (tinympc_get_stream) or a synchronous verb. */
int tinympc_get_solution_device_ptrs(tinympc_solver *s, const double **d_x, const double **d_u);

/* Closed-loop SESSION (single-instance handles): the reference's control loops call set_x0 -> solve -> get_solution
 * once per tick (examples/cartpole_example_mpc.m:36-44); every such tick pays a kernel launch and a stream
 * synchronisation (~10 us of a ~15 us tick). In a session the solve kernel is launched ONCE and stays resident: it polls
 * a mailbox for the next x0 (a line of device memory the host writes through the PCIe BAR; pinned host memory where the device's
 * memory is not host-visible), runs the warm-started solve with the ADMM state kept in registers, sends the first controls to
 * pinned host memory at once -- tinympc_session_step returns with them (a quadrotor N=50 tick: 6 us) -- and then the solution and
 * a completion stamp, which tinympc_get_solution / _get_stats wait for.
 *   tinympc_session_begin   settings, bounds, cache are frozen for the session; references may change between ticks
 *                           (tinympc_set_x_ref / _set_u_ref: picked up by the next step)
 *   tinympc_session_step    x0 in (nx), first controls out (nu); tinympc_get_solution / _get_stats work as usual
 *   tinympc_session_end     stops the kernel; the handle continues with ordinary solves from the same ADMM state.
 * Any other verb that needs the device ends the session implicitly, and so do tinympc_update_settings,
 * tinympc_set_cone_constraints and tinympc_set_linear_constraints (the resident kernel carries the settings and
 * families it was launched with): call tinympc_session_begin again afterwards. The resident kernel leaves on its own
 * after 2 s without a command (a crashed host does not leave it spinning); the next step restarts it transparently.
 * While the resident kernel spins, calls that synchronise the whole DEVICE wait for it -- up to the 2 s idle time-out.
 * This library's own such calls (tinympc_setup / tinympc_reset of ANOTHER handle on the device: hipMalloc / hipFree) first
 * send the resident kernels of the device home; their sessions stay open and the next tinympc_session_step starts the
 * kernel again (a few milliseconds, once). Calls from outside the library (hipDeviceSynchronize, torch.cuda.synchronize,
 * somebody else's hipMalloc) cannot be seen coming: end the session before them. The resident kernel is the variant of the
 * kernel the handle's launches run on (layout F where that is compiled in, was asked for with tinympc_prepare, or carries the cone /
 * linear families; layout C otherwise): its results are identical, bit for bit, to the same ticks issued as tinympc_mpc_step_batch
 * calls. (Only where layout F has no resident kernel for a configuration its launches run on does the session fall back to layout
 * C's, whose results differ from layout F's in the last bits: the carries of its chunks round differently.) */
int tinympc_session_begin(tinympc_solver *s);
int tinympc_session_step(tinympc_solver *s, const double *x0, double *u0_out);
int tinympc_session_end(tinympc_solver *s);
/* Resident solves (an extension, off by default): after tinympc_set_resident(h, 1) the reference's own per-tick sequence
 * tinympc_set_x0 -> tinympc_solve -> tinympc_get_solution / tinympc_get_stats runs on the resident session kernel instead of one launch per
 * solve (a quadrotor N=50 tick: 6 us instead of 15). Results are bit-identical to launched solves. Single-instance handles with nx+nu <= 16
 * and no adaptive rho; elsewhere solves are launched as before. Any verb that needs the device (new bounds, settings, ...) sends the
 * resident kernel home, the next solve starts it again; it also leaves by itself after 2 s without a solve. While it is resident it occupies
 * one compute unit and a DEVICE-wide synchronisation of other code in the process (hipMalloc, hipDeviceSynchronize) waits for it -- up to
 * that idle time-out: the reason this is not the default. enable = 0 ends it. */
int tinympc_set_resident(tinympc_solver *s, int enable);

/* Launch the solve without waiting (same kernel as tinympc_solve); pair with tinympc_synchronize. Every verb
 * that changes an input of the launch in flight (set_x0, mpc_step, ... -- on single-instance handles x0 lives in
 * pinned host memory that the kernel reads directly) waits for the launch first, so the sequence solve_async ->
 * set_x0 (next tick) -> synchronize is safe for every batch size. */
int tinympc_solve_async(tinympc_solver *s);
int tinympc_synchronize(tinympc_solver *s);
/* Synchronous solve that also reports the kernel's duration measured with HIP events recorded on
 * the handle's stream immediately around the launch. */
int tinympc_solve_timed(tinympc_solver *s, float *kernel_ms);

/* Throughput form of the timed solve: queue the launch on the handle's stream and return at once; every queued launch records its
 * own HIP event pair around the solve kernel. tinympc_collect_kernel_ms waits for the stream and returns the kernel durations of
 * the launches queued since the last collect, in order (*count; an error if they exceed `capacity`, at most 4,096). Between two
 * queued solves the caller may queue tinympc_reset_workspace (stream-ordered, returns at once). tinympc_set_x0_batch_device is
 * correct there too but NOT asynchronous: it waits for the handle's stream -- i.e. for every launch queued so far -- before it
 * returns, because the caller may free or reuse d_x0s as soon as it does; a pipeline that wants new x0 per queued solve
 * without draining the queue keeps them in one device array and switches by offset before queueing. Host readers
 * (get_solution ...) synchronise as always. Batched handles outside a session only. */
int tinympc_solve_queued(tinympc_solver *s);
int tinympc_collect_kernel_ms(tinympc_solver *s, float *kernel_ms, int capacity, int *count);

/* One closed-loop control tick for every instance of the handle (the loop of
 * examples/cartpole_example_mpc.m:36-44 / rocket_landing_constraints.m:86-121 as ONE call): upload the
 * measured states x0s (nx x batch), run the warm-started solve, download the first control of each
 * instance into u0_out (nu x batch). One stream submission and one synchronisation instead of three
 * synchronous verbs: up to 256 instances the kernel reads x0 from and writes the first controls to pinned
 * host memory itself (no copy engine involved), larger batches go through two async copies. Results are
 * identical to tinympc_set_x0_batch + tinympc_solve + tinympc_get_first_controls_batch.
 * (Single-instance handles get the same treatment for the plain verbs: tinympc_set_x0 only fills a pinned
 * buffer the next launch reads, and tinympc_get_solution / tinympc_get_stats after a solve are host copies.) */
int tinympc_mpc_step_batch(tinympc_solver *s, const double *x0s, double *u0_out);

/* Closed-loop rollout on the device (batched handles outside a session; no reference counterpart). A closed-loop study is `ticks`
 * times: solve, apply the first control to a plant, measure. With the plant on the host every tick is one upload of x0, one download
 * of the first controls and one stream synchronisation around the solve; here the plant runs behind the solve on the handle's
 * stream (k_plant_step, csrc/tinympc_rollout.hip) and the state never leaves the device.
 *
 * tinympc_rollout_batch starts from the x0 the handle holds (tinympc_set_x0_batch / _device) and queues, for t = 0 .. ticks-1,
 * exactly what a tinympc_mpc_step_batch tick launches (the warm-started solve, x0 read from device memory) and then, for every
 * instance b,
 *     x_log[b][:, t] = x0[b],  u_log[b][:, t] = u,  iter_log[b][t],  status_log[b][t]     (u: the first control of that solve)
 *     x0[b] <- A_p x0[b] + B_p u + f_p + disturbance[b][:, t]                              (and x_log[b][:, ticks] after the last tick)
 * and the reference tracks' auto-advance where it is on (tinympc_set_ref_auto_advance). No host copy and no synchronisation
 * between ticks, no graph capture; one synchronisation at the end, then the requested logs are copied out of device buffers the
 * handle keeps (grown on demand, freed with the handle). Afterwards x0 holds the final state, and the ADMM state, the tracks' steps
 * and every getter are as after the same ticks issued one by one (tinympc_solve + tinympc_plant_step_batch, bit for bit).
 *   plant    A_p, B_p, f_p: the override of tinympc_set_plant_batch; else the instance's own model while per-instance models are on
 *            (tinympc_set_model_batch); else the handle's shared A, B, fdyn.
 *   order    per row one chain of fused multiply-adds, started from f_p (zero where there is none), over A_p's columns ascending,
 *            continued over B_p's columns ascending; then + disturbance. Fixed: results are reproducible bit for bit.
 *   layout   instance-major, the layout of the reference tracks: x_log nx x (ticks+1) x batch (instance b's block at
 *            b nx (ticks+1)), u_log nu x ticks x batch, iter_log and status_log ticks x batch (instance b's row at b ticks),
 *            disturbance nx x ticks x batch (NULL: none). A rollout's x_log can be handed as it is to
 *            tinympc_set_x_ref_track_batch / _device of another handle (T = ticks+1).
 *   logs     any member, or logs itself, may be NULL: that log is not written.
 *   gpu_ms   (may be NULL) one event pair around the whole queue, in milliseconds.
 * tinympc_rollout_batch_device writes the logs to, and reads the disturbance from, caller-owned device memory on the handle's GPU
 * (d_logs is a host struct of device pointers). It returns once the work is QUEUED: the caller orders its reads behind the handle's
 * stream (tinympc_get_stream, or tinympc_synchronize) and keeps the buffers alive until then.
 * tinympc_plant_step_batch queues the plant step once, without logs -- the same kernel and arithmetic: x0 <- plant(x0, first controls
 * of the last solve) + disturbance (host memory, nx x batch, or NULL). For callers that want to look at every tick.
 * Refusals (nothing is queued or changed): TINYMPC_ERR_INVALID_INPUT for ticks < 1, for max_iter < 1 (a tick that writes no control
 * cannot be rolled out) and for anything but the handle's GPU's memory handed to the _device form; TINYMPC_ERR_UNSUPPORTED for
 * single-instance handles that answer through pinned host memory and inside a session; and whatever a launch of the current
 * configuration refuses, with the launch's own code and message, before tick 0. */
typedef struct { double *x_log, *u_log; int *iter_log, *status_log; } tinympc_rollout_logs;   /* any member may be NULL */
int tinympc_rollout_batch(tinympc_solver *s, int ticks, const double *disturbance, const tinympc_rollout_logs *logs, float *gpu_ms);
int tinympc_rollout_batch_device(tinympc_solver *s, int ticks, const double *d_disturbance, const tinympc_rollout_logs *d_logs);
int tinympc_plant_step_batch(tinympc_solver *s, const double *disturbance);

/* A plant that differs from the controller's model (model-mismatch and robustness studies): A is nx x nx x count, B nx x nu x count,
 * f nx x count or NULL (no affine term), for instances first .. first+count-1; column-major blocks, one per instance. The first call
 * must name the whole batch, later calls may replace sub-ranges. Everything is validated before anything is written (finite values;
 * the _device form on the device, one flag read back). The controller is never touched: cache, operators, table rows and kernel
 * plan stay as they are. tinympc_clear_plant_batch returns to the model's own plant. Batched handles only. */
int tinympc_set_plant_batch(tinympc_solver *s, const double *A, const double *B, const double *f, int first, int count);
int tinympc_set_plant_batch_device(tinympc_solver *s, const double *d_A, const double *d_B, const double *d_f, int first, int count);
int tinympc_clear_plant_batch(tinympc_solver *s);

/* Rollout metrics: what a closed-loop study wants of a rollout is a few numbers per instance, not every state of every tick. While
 * the metrics are on, every plant step the handle queues (tinympc_rollout_batch / _device of any length, in any number of calls, and
 * tinympc_plant_step_batch) runs the scored variant of k_plant_step, which moves one row of 8 doubles per instance on, in device
 * memory the handle owns ([batch][8], allocated by the first call, freed with the handle). A scored rollout without logs moves
 * 64 bytes per instance to the host instead of the logs. With x = x0[b] before the step, u the first control of the solve that
 * just ran, xr / ur the reference that solve tracked at knot 0, lo / hi its bounds at knot 0, e = x - xr, d = u - ur, and t the
 * steps since the reset:
 *   [0] steps accumulated
 *   [1] cost: the running sum of qx_i (e_i e_i) over the state rows ascending, then ru_j (d_j d_j) over the input rows ascending
 *   [2] max over steps and rows of max(0, lo_i - x_i, x_i - hi_i)      (0 while en_state_bound is off)
 *   [3] the same for u against the input bounds                          (0 while en_input_bound is off)
 *   [4] sum of the iteration counts      [5] most iterations of one step      [6] steps whose status is not TINYMPC_STATUS_SOLVED
 *   [7] settle step: t + 1 of the last step with max_i |e_i| > settle_tol; 0 if there was none, or if settle_tol <= 0
 * Counts are stored as doubles and are exact.
 *   order    slot 1 is ONE chain per step: it starts from the stored cost and adds one term per row, state rows ascending, then input
 *            rows ascending; every product is rounded once (e e, then times the weight) and nothing is contracted into the add.
 *            Fixed: the rows are reproducible bit for bit, a rollout of T ticks equals two of T/2, and a sequential float64
 *            restatement reproduces them exactly.
 *   xr, ur   what the solve used: a half in track mode, column min(step[b], T - 1) of the instance's track, read before the
 *            auto-advance; else the instance's own reference (tinympc_set_x_ref_batch / _u_ref_batch), column 0; else the shared one,
 *            column 0. lo, hi: the instance's bounds where tinympc_set_bound_constraints_batch is on, else the shared ones, column 0.
 * tinympc_set_rollout_metrics turns the metrics on (or replaces the weights: qx nx values, ru nu values, shared by the batch) and
 * zeroes every row; tinympc_reset_rollout_metrics zeroes the rows, queued on the handle's stream; tinympc_clear_rollout_metrics turns
 * them off: steps run the plain kernel again. tinympc_get_rollout_metrics copies the rows out (8 x batch, row b at 8 b) and
 * synchronises; the _device_ptr form hands out the rows themselves: order reads behind the handle's stream. x0, the logs, the ADMM
 * state and every getter are bit for bit what they are without the metrics.
 * Refusals (nothing is queued or changed): TINYMPC_ERR_UNSUPPORTED for single-instance handles that answer through pinned host memory
 * and inside a session; TINYMPC_ERR_INVALID_INPUT for a NULL qx or ru, a weight that is negative or not finite, a settle_tol that is
 * not finite, and for get / reset / device_ptr while the metrics are off. */
typedef struct { const double *qx, *ru; double settle_tol; } tinympc_rollout_score;  /* qx: nx weights, ru: nu weights, shared by the batch */
int tinympc_set_rollout_metrics(tinympc_solver *s, const tinympc_rollout_score *score);  /* on (or re-weighted), and reset */
int tinympc_reset_rollout_metrics(tinympc_solver *s);                                   /* zero every row, queued on the stream */
int tinympc_clear_rollout_metrics(tinympc_solver *s);                                   /* off: steps run the plain kernel again */
int tinympc_get_rollout_metrics(tinympc_solver *s, double *out);                        /* 8 x batch, synchronises */
int tinympc_get_rollout_metrics_device_ptr(tinympc_solver *s, const double **d_rows);    /* ordered behind the handle's stream */

/* Rollout noise: seeded process and measurement noise for Monte-Carlo studies, drawn on the device by the plant step itself -- no
 * nx x ticks x batch disturbance to draw on the host and upload. While the noise is on, every plant step the handle queues
 * (tinympc_rollout_batch / _device of any length, in any number of calls, and tinympc_plant_step_batch) runs a noisy variant of
 * k_plant_step, scored as well while the metrics are on, with the handle's noise tick, which then moves on by one.
 *   draw     n(g, tick, r, stream): a standard normal that is a pure function of the seed, the instance's global index
 *            g = first_instance + b, the noise tick, the state row r and the stream (0: process, 1: measurement). Philox4x32-10
 *            (multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85) with key (seed & 0xffffffff, seed >> 32) and
 *            counter (g, tick, r, stream) gives the words o0..o3; u1 = ((o0 >> 5) 2^26 + (o1 >> 6) + 1) 2^-53 in (0, 1],
 *            u2 = ((o2 >> 5) 2^26 + (o3 >> 6)) 2^-53 in [0, 1); n = sqrt(-2 log(u1)) * cos(6.283185307179586 * u2), every operation
 *            rounded once, nothing contracted; |n| <= 8.58. It depends on nothing else: not on the layout, not on how a rollout is cut
 *            into calls (T ticks equal T/2 + T/2), not on how a fleet is cut into handles (a shard with its first_instance draws what the
 *            same instances draw unsharded).
 *   step     with x the TRUE state (x_log and the metrics see this x), sw / sv the scales of the row:
 *              x+ = (A_p x + B_p u + f_p + w[b][:, t]) + (sw_r n(g, tick, r, 0))      the plain step's chain and disturbance, then the
 *                                                                                      process term: product rounded, then the add
 *              x0[b][r] = x+ + (sv_r n(g, tick, r, 1))                                 the measurement the NEXT solve reads
 *            Without measurement noise x0 is the true state as ever. With it the handle keeps the true state beside x0, in memory it
 *            owns; the first tick's measurement is whatever x0 holds (a caller who wants it noisy adds its own). A verb that writes x0
 *            from outside (tinympc_set_x0_batch / _device, tinympc_set_x0, tinympc_mpc_step_batch) restarts the true state of the
 *            instances it names from what it wrote.
 * tinympc_set_rollout_noise takes standard deviations per state row -- nx values shared by the batch, or nx x batch (instance b at
 * nx b) with per_instance != 0; either array may be NULL: that family is off and nothing is drawn for it --, copies them to device
 * memory the handle owns, and sets the noise tick to 0. A level sweep is one handle and one launch. tinympc_clear_rollout_noise turns
 * the noise off: steps run the plain or scored kernels again, and where measurement noise was on the true state goes back into x0
 * (queued), so the loop continues from it. tinympc_get_rollout_noise regenerates, by the step's own device function, what the steps of
 * ticks first_tick .. first_tick + ticks - 1 add: w_out = sw_r n(., 0), v_out = sv_r n(., 1), each nx x ticks x batch in the
 * disturbance's layout; either may be NULL, a family that is off yields zeros. A noise-free handle given w_out as its disturbance
 * reproduces a process-noise rollout bit for bit. tinympc_get_plant_state_batch copies out the true state (nx x batch): the state
 * beside x0 while measurement noise is on, else x0; it synchronises.
 * Refusals (nothing is queued or changed): TINYMPC_ERR_UNSUPPORTED for single-instance handles that answer through pinned host memory
 * and inside a session; TINYMPC_ERR_INVALID_INPUT for a NULL struct, both arrays NULL, a scale that is negative or not finite,
 * first_instance + batch > 2^32, ticks < 1, a step (or a replay) whose tick would reach 2^32, and for get_rollout_noise / clear while
 * the noise is off. */
typedef struct { const double *process, *measurement; int per_instance; unsigned long long seed, first_instance; } tinympc_rollout_noise;
int tinympc_set_rollout_noise(tinympc_solver *s, const tinympc_rollout_noise *noise);
int tinympc_clear_rollout_noise(tinympc_solver *s);
int tinympc_get_rollout_noise(tinympc_solver *s, unsigned long long first_tick, int ticks, double *w_out, double *v_out);
int tinympc_get_plant_state_batch(tinympc_solver *s, double *x_out);

/* Launch geometry of the solve kernel, for reports: lanes per instance, instances per wavefront,
 * workgroups in the grid, dynamic LDS bytes per workgroup, and whether the per-knot bound/reference
 * tables are LDS-resident. Any pointer may be NULL. */
int tinympc_get_launch_info(tinympc_solver *s, int *lanes_per_instance, int *instances_per_wave,
                            int *workgroups, int *lds_bytes, int *tables_in_lds);

/* Which solve kernel the handle's next launch uses: 'A' (all ADMM state in LDS, one wavefront per workgroup), 'B' (V
 * L2-resident in HBM, four wavefronts per workgroup), 'C' (one instance per workgroup, horizon swept in 16 concurrent
 * chunks; batches up to 768 and every single solve), 'D' (horizon unrolled at compile time, state in registers; large
 * batches), 'E' (as D with the horizon cut across the wavefronts of a workgroup: cone / linear families at long horizons),
 * 'F' (the latency kernel specialised at run time: up to 32 chunks on two wavefronts per SIMD; the families at small batches),
 * 'M' (64 < nx+nu <= 512 on the FP64 matrix cores). The environment variable TINYMPC_LAYOUT=A|B|C|D|E|F overrides the choice.
 * 0 for a NULL handle. */
int tinympc_get_layout(tinympc_solver *s);

/* Where the kernel of the handle's CURRENT configuration comes from, as text: "compiled-in layout=X", or for the run-time
 * specialised kernels (layouts D and E) "compiled ..." / "disk-cache ..." with the code object's register count, scratch and LDS
 * bytes, or "refused(<reason>)" when the specialiser declined (plan overflow, spills, compile error, TINYMPC_JIT=0) and the
 * launch falls back to a generic kernel. Refusals are also printed once to stderr (TINYMPC_JIT_QUIET=1 silences them).
 * " slot-refill" is appended when the launch uses layout D's slot-refill variant: a batch larger than the device holds at once
 * (8,192 instances of 16 lanes on MI355X) runs as ONE resident set of wavefronts, and a 16-lane row whose instance has finished
 * (converged, or max_iter) is written back and given the next instance of the batch while the rest of its wavefront keeps
 * iterating -- a wavefront then costs the sum of what its rows worked instead of four times its slowest instance. Results are
 * bit-identical to the plain kernel's. Taken whenever the tolerances can be met (with forced iteration counts there is nothing to
 * balance); TINYMPC_REFILL=0 switches it off, =1 takes it for any batch beyond one resident set. The box path of the 16-lane
 * shapes: handles whose instances share one reference and one box, and handles with one goal and / or one box per instance
 * (tinympc_set_x_ref_batch / _u_ref_batch / _set_bound_constraints_batch with one column per instance: layout D's goal form,
 * " goal slot-refill" -- a row that takes an instance takes its goal and box with it), and, after tinympc_prepare, handles on layout
 * D's per-instance trajectory form (trajectories, tracks) and / or per-knot bounds form (" per-instance-trajectories slot-refill",
 * " per-knot-bounds slot-refill" -- the row also restages its column of its wavefront's reference / clamp rows; a resident set is that
 * form's own: 4,096 instances where it runs one wavefront per SIMD, e.g. the quadrotor's trajectories at N = 50). Not with
 * per-instance models, rho, linear rows or cone slopes, the families, adaptive rho or the zero-copy tick. */
int tinympc_get_jit_info(tinympc_solver *s, char *buf, int len);

/* Decide (and, where needed, specialise -- seconds the first time) the solve kernel for the handle's CURRENT configuration:
 * bounds / references that vary over the horizon, cone / linear families, adaptive rho and slot refill select variants that are
 * otherwise built at the first launch that needs them. Call it once after the constraints and settings are in place to keep that
 * one-off cost out of the first real-time tick. It also tells the library that run-time specialisation is welcome on this handle:
 * a single instance / small batch of a shape that is not compiled in then runs on the structure-specialised latency kernel (layout
 * F: 5-25 % fewer microseconds per iteration than the generic latency kernel, resident session included) instead of staying on the
 * generic one, which needs no compiler; and a batch with per-instance models (tinympc_set_model_batch, in either order) runs on layout
 * D's per-instance model form where one exists instead of layout A, and a batch with per-instance linear rows
 * (tinympc_set_linear_constraints_batch, in either order) on layout D's per-instance linear-row form likewise; and a batch with
 * per-instance reference trajectories or tracks (tinympc_set_x_ref_batch / _u_ref_batch with cols = N / N-1, the track verbs, in either
 * order) on layout D's per-instance trajectory form -- nx+nu <= 16, bounds constant over the horizon, no per-instance models or rho, no
 * cone / linear families, no adaptive rho, a horizon whose reference rows fit a wavefront's LDS share; and a batch with BOTH
 * per-instance linear rows (or rows per knot, or cone slopes) and per-instance trajectories or tracks on the linear-row form that reads
 * every wavefront's own reference rows, where rows and references fit the wavefront's LDS share together (a trajectory shared by the
 * batch through tinympc_set_x_ref / _set_u_ref is not one of these: layout A); and a batch with box bounds per knot and per instance
 * (tinympc_set_bound_constraints_batch with cols = N, in either order), or with shared per-knot bounds beside per-instance trajectories
 * or tracks, on layout D's per-knot bounds form under the same conditions, where the clamp rows fit the wavefront's LDS share too;
 * otherwise layout A as without this call. Where the trajectory or per-knot bounds form is already the handle's and its batch lies
 * beyond one resident set, the form's slot-refill variant is built here as well. No reference
 * counterpart (the reference has one code path). */
int tinympc_prepare(tinympc_solver *s);

/* The HIP stream of the handle as an opaque pointer (hipStream_t). */
void *tinympc_get_stream(tinympc_solver *s);

#ifdef __cplusplus
}
#endif
#endif /* TINYMPC_HIP_H */
