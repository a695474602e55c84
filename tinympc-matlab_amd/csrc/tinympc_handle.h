// tinympc_handle.h -- the solver handle behind the C ABI (include/tinympc_hip.h) and the host-side helpers its translation units
// share:  tinympc_capi.hip (the verbs), tinympc_handle.hip (buffers, derived tables, the families' description),
//         tinympc_plan.hip (WHICH kernel a launch runs -- one LaunchPlan, chosen in one function -- and the launch itself),
//         tinympc_session.hip (the resident closed-loop session).
// Host-side bookkeeping only: every number the solver produces is computed by the kernels; there is no CPU fallback anywhere.
#pragma once
#include "tinympc_hip.h"
#include "tinympc_hip_bench.h"  // (the diagnostics the product library itself exports)

#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <string>
#include <vector>

#include "tinympc_device.h"
#include "tinympc_host.h"

#define HIP_TRY(expr)                                                                                     \
    do {                                                                                                  \
        hipError_t e__ = (expr);                                                                          \
        if (e__ != hipSuccess)                                                                            \
            return tinympc::fail(TINYMPC_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), \
                                 __FILE__, __LINE__);                                                     \
    } while (0)

namespace tinympc {

struct Settings {  // TinySettings (types.hpp:61-74) + the newer flags (bindings.cpp:583-586)
    double abs_pri_tol, abs_dua_tol;
    int max_iter, check_termination;
    int en_state_bound, en_input_bound;
    int en_state_soc, en_input_soc, en_state_linear, en_input_linear;
    int adaptive_rho;
    double adaptive_rho_min, adaptive_rho_max;
    int adaptive_rho_enable_clipping;
};

constexpr double kBoundInf = 1e17;  // TinyMPC.m:261-264
// Every pinned buffer the kernels and the host exchange data through WHILE a kernel runs (completion flags, the session
// mailbox, references re-read by a resident kernel) is allocated hipHostMallocCoherent: with the default flags the
// GPU may keep host lines in its L2 until the kernel ends, and a resident kernel then polls a stale copy forever.
constexpr int kZeroCopyTickMax = 256;   // mpc_step: up to this many instances exchange x0 / u0 through pinned host memory
constexpr int kZeroCopyTickMaxD = 1 << 30;  // ... on layout D: any batch (measured: tools/tick_latency.py)
constexpr int kLayoutEBatchMin = 260;   // families at horizons layout D cannot hold: from here on layout E (4 instances per CU, the whole
                                        // state on chip) passes the latency kernel (1 instance per CU); measured, profiles/r03_rocket_sweep.txt
constexpr int kLayoutCBatchMax = 768;  // above this the batch-oriented layouts win (profiles/r02_layout_sweep.txt: layout D with four
                                       // wavefronts per workgroup passes the latency kernel between 512 and 1,024 instances)


}  // namespace tinympc

// Per-instance references and bounds of a batched handle. Each mode -- the x half of the references, the u half, the bounds -- is on from
// its first per-instance verb until the shared verb (tinympc_set_x_ref / _set_u_ref / _set_bound_constraints); instances the verbs did
// not name hold the shared value of the moment the mode began. The rows the solve kernels read (SolveParams::iref_lr / iref_pn / ibnd)
// are rebuilt at the next launch for the instances in [dirty_lo, dirty_hi) -- all of them when the shared tables were rebuilt (new
// references, bounds or cache). One interval: two small updates far apart rebuild the instances between them too (a rebuild is one
// element-wise kernel over the interval). A mode's rows hold the shared values where it is off.
struct InstState {
    bool x = false, u = false, bounds = false;
    // ... every instance's value of that mode is constant over the horizon. Sticky until the mode ends: a trajectory that is later
    // replaced by goals keeps the handle on layout A (nothing looks at the whole batch's data again)
    bool x_const = false, u_const = false, bounds_const = false;
    int d_goal = -1;  // the run-time specialised goal kernel (16 lanes beyond the compiled-in shapes, 32 / 64 lanes): -1 not asked yet, 0 no, 1 yes
    // layout D's per-instance trajectory form (ITRAJ: 16 lanes, compiled in or run-time specialised; trajectories and tracks of a handle that
    // called tinympc_prepare, bounds constant over the horizon): -1 not asked yet, 0 no (the horizon's rows do not fit a wavefront's LDS
    // share, or the specialiser refused: the mode stays on layout A), 1 yes
    int d_traj = -1;
    // layout D's per-knot bounds form (IKBND, with ITRAJ where a reference half is a per-instance trajectory or track: 16 lanes, compiled in or
    // run-time specialised; bounds that vary over the horizon on a handle that called tinympc_prepare): -1 not asked yet, 0 no (the
    // specialiser refused), 1 yes, 2 no plan (the horizon's clamp rows do not fit a wavefront's LDS share: the mode stays on layout A and
    // nothing was refused). The answer is the one for d_kbnd_traj, the ITRAJ variant it was asked for.
    int d_kbnd = -1;
    bool d_kbnd_traj = false;
    // ... the form reads layout A's clamp rows (bnd): from its first launch on they are built in every mode, from the shared bounds too
    bool bnd_always = false;
    // every instance's value, column-major [batch] blocks of nx x N (Xi, xmin, xmax) / nu x (N-1) (Ui, umin, umax)
    double *Xi = nullptr, *Ui = nullptr, *xmin = nullptr, *xmax = nullptr, *umin = nullptr, *umax = nullptr;
    double *lr = nullptr, *pn = nullptr;     // linref rows (inst_lr_doubles), pNref [instance][W]
    double *lrg = nullptr, *bndg = nullptr;  // knot 0's linref [instance][W] and lo | hi rows (layout D's goal form)
    double *bnd = nullptr;                   // layout A's lo | hi rows (inst_bnd_doubles; bounds mode)
    double *stage = nullptr;                 // device staging of one-column host input
    // Per-instance models (tinympc_set_model_batch, tinympc_set_rho_batch): on from the first call of either until
    // tinympc_clear_model_batch. Every instance's model (A | B | fdyn | Qd | Rd, the diagonals + rho as PrecomputeParams wants them), its
    // LQR cache and its operator block, each array [batch][block]; filled from the shared model, cache and operators when the mode
    // begins, recomputed for the instances a call names (batched precompute + operator builder, inside the call). The store also keeps
    // the RAW cost diagonals (mQ0 | mR0) and every instance's rho (mrho: the handle's until tinympc_set_rho_batch names the instance):
    // Qd_b = Q0_b + rho_b is formed from them by one addition, whichever verb came last, so the two verbs commute bit for bit. The mode runs on layout A's InstModels variant, always with the
    // per-instance reference and clamp rows, which are then built from the instance's own Pinf and cost diagonals -- or, once the caller
    // has asked for specialised kernels (tinympc_prepare) and references and bounds are constant over the horizon, on layout D's IMOD form.
    bool models = false;
    int d_models = -1;  // layout D's per-instance model form (16 lanes; compiled in or run-time specialised): -1 not asked yet, 0 no, 1 yes
    bool rho_verb = false;  // ... and tinympc_set_rho_batch was among the calls (the refusals name it)
    double *mA = nullptr, *mB = nullptr, *mf = nullptr, *mQd = nullptr, *mRd = nullptr;
    double *mQ0 = nullptr, *mR0 = nullptr, *mrho = nullptr;  // raw diagonals [batch][nx] / [batch][nu], rho [batch] (SolveParams::rho_inst of the model kernels)
    int *mflag = nullptr;                    // one flag: the device-side validation of tinympc_set_rho_batch_device
    double *cK = nullptr, *cP = nullptr, *cQuu = nullptr, *cAm = nullptr, *cAPf = nullptr, *cBPf = nullptr;
    int *cinfo = nullptr;                    // [batch][4]: Riccati steps (and the rows kernel's clocks)
    double *ops = nullptr;                   // [batch][ops_doubles(W, KT)]: SolveParams::ops of the InstModels variant
    double *mscratch = nullptr;              // working sets of k_precompute's batched form where they do not fit LDS
    double *mstage = nullptr;                // device staging of the cost diagonals (host input)
    // Reference tracks (tinympc_set_x_ref_track_batch / _u_ref_track_batch): a half in track mode is a half with per-instance
    // trajectories (x / u above is on, x_const / u_const off) whose rows are built from a store LONGER than the horizon -- Xt / Ut,
    // [batch][T][rows], T knots per instance -- and the instance's step: knot kn of instance b is column min(steps[b] + kn, T - 1)
    // (k_build_inst_tables). One step per instance serves both halves; the step array stays when a half leaves the mode, and the
    // store of a half that left is kept for the next track (xt_cap / ut_cap doubles). Single-instance handles keep the track on the
    // host (hXt / hUt, hstep) and forward the current window through the shared reference verbs.
    bool x_track = false, u_track = false;
    int Tx = 0, Tu = 0;
    double *Xt = nullptr, *Ut = nullptr;
    size_t xt_cap = 0, ut_cap = 0;
    int *steps = nullptr;
    int auto_advance = 0;  // tinympc_mpc_step_batch adds this to every step after its solve (0: off)
    std::vector<double> hXt, hUt;
    int hstep = 0;
    bool tracks() const { return x_track || u_track; }
    // Per-instance linear rows (tinympc_set_linear_constraints_batch): on from the first call until tinympc_set_linear_constraints. The row
    // COUNTS (lin_nlx, lin_nlu; also the handle's n_lin_x / n_lin_u while the mode is on) belong to the batch, the values to the
    // instance: lrows is the store the kernel reads, SolveParams::ilin, [group][3 lin_nl][64] with lin_nl = max(lin_nlx, lin_nlu)
    // (k_build_inst_lin; instances the verb never named hold the shared rows of the moment the mode began). Nothing else is kept: the
    // store IS the rows, written inside the call. The mode runs on layout A's InstFamilies variant, always with the per-instance
    // reference and clamp rows -- or, once the caller has asked for specialised kernels (tinympc_prepare), bounds are constant over the
    // horizon, every reference half is constant over the horizon or a per-instance trajectory / track, and the cones are ones layout D's
    // families kernel takes, on layout D's ILIN form (lin_wants_d; with trajectories: ILIN with ITRAJ, lin_d_traj).
    bool lin = false;
    int lin_nlx = 0, lin_nlu = 0, lin_nl = 0;
    // ... and its third state, rows per KNOT (tinympc_set_linear_constraints_knots_batch): lin_knots = N while it is on, 0 otherwise. The store
    // then holds N slots of rows per group (inst_fam_block_doubles), the mode runs on layout A's InstFamiliesKnots variant -- or, under
    // lin_wants_d's conditions and where its per-wavefront plan holds the N slots, on the per-knot variant of layout D's ILIN form --, and a whole-batch tinympc_set_linear_constraints_batch or the shared verb ends it.
    int lin_knots = 0;
    // layout D's per-instance linear-row form (16 lanes; compiled in or run-time specialised on the shape AND lin_nl): -1 not asked yet,
    // 0 no, 1 yes -- the answer for d_lin_nl rows; another count (a whole-batch call) makes it unknown again (resolve_plan). The cones are
    // no part of the specialisation: whether their structure is one the form takes is asked at every launch (lin_wants_d).
    int d_lin = -1, d_lin_nl = 0;
    bool d_lin_cones = false;                // ... and for the slope half on / off (ICONE: the form that reads the slope per instance)
    int d_lin_knots = 0;                     // ... and for rows per knot (lin_knots of the answer) or rows constant over the horizon (0)
    bool d_lin_traj = false;                 // ... and for per-instance trajectories / tracks (ITRAJ with ILIN: the wavefront's own linref rows) or references constant over the horizon
    double *lrows = nullptr;
    size_t lrows_cap = 0;                    // doubles lrows was allocated for
    double *lstage = nullptr;                // device staging of host input (the shared rows of a sub-range first call: a block of their own, freed in the call)
    size_t lstage_cap = 0;
    // Per-instance cone slopes (tinympc_set_cone_slopes_batch): the other half of the same mode -- on from the first call until
    // tinympc_set_cone_constraints. The cones' STRUCTURE stays the handle's; craw keeps every instance's slopes, [batch][n_cone_x + n_cone_u]
    // in list order (instances the verb never named: the shared slopes of the moment the half began). The kernels read the store's slope
    // vectors in front of each group's rows in lrows, which refresh_inst_families rebuilds from craw -- or, while only the row half is on,
    // from the shared slopes -- whenever the slopes, the structure or an enable flag changed (the rounds follow the enabled sides).
    // While only THIS half is on the store's rows are the shared rows, copied for every instance (fam_rows_nl of them; one absent row on a
    // handle without linear rows).
    bool cones = false;
    bool fam() const { return lin || cones; }  // the per-instance families mode: either half
    double *craw = nullptr;
    double *cshared = nullptr;               // the shared slopes cx | cu on the device (the row half alone)
    size_t craw_cap = 0;
    bool slopes_dirty = true, shared_rows_dirty = true;  // the store's slope vectors / its copy of the shared rows are out of date
    int fam_rows_nl = 0;                     // rows per instance the store holds now (SolveParams::ilin_nl; 0: no store yet)
    int fam_rows_knots = 0;                  // ... and its knot slots per group (SolveParams::ilin_knots; 0: rows constant over the horizon)
    int dirty_lo = 0, dirty_hi = 0;
    bool refs() const { return x || u; }
    const double *lr_rows() const { return lr + (size_t)tinympc::INST_LR_PAD * 64; }  // SolveParams::iref_lr on layout A
    void mark(int lo, int hi) {
        if (dirty_lo >= dirty_hi) { dirty_lo = lo; dirty_hi = hi; }
        else { dirty_lo = lo < dirty_lo ? lo : dirty_lo; dirty_hi = hi > dirty_hi ? hi : dirty_hi; }
    }
};

struct tinympc_solver {
    int nx = 0, nu = 0, N = 0, batch = 0, device = 0;
    int W = 0, KT = 0, IPW = 0, groups = 0;
    double rho = 0.0;
    tinympc::Settings st{};
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::vector<hipEvent_t> ring_ev;  // tinympc_solve_queued: one event pair per queued launch (2 i, 2 i + 1)
    int ring_count = 0;               // pairs recorded since the last tinympc_collect_kernel_ms
    // problem + cache
    double *dA = nullptr, *dB = nullptr, *dfdyn = nullptr, *dQd = nullptr, *dRd = nullptr;
    double *dKinf = nullptr, *dPinf = nullptr, *dQuu = nullptr, *dAmBKt = nullptr, *dAPf = nullptr, *dBPf = nullptr;
    double *dscratch = nullptr;
    int *dinfo = nullptr;
    // the .m class's own Riccati helpers (compute_cache_terms / solve_lqr / compute_sensitivity_autograd)
    double *dQfull = nullptr, *dRfull = nullptr, *dlqr_scratch = nullptr, *dlqr_out = nullptr;  // dlqr_out: 3 x cache_doubles()
    // adaptive rho: sensitivities dKinf/drho, dPinf/drho (zeros until set), kernel tables, per-instance rho
    double *ddK = nullptr, *ddP = nullptr, *dadapt = nullptr, *drho_inst = nullptr;
    size_t cache_doubles() const { return (size_t)nu * nx + (size_t)2 * nx * nx + (size_t)nu * nu; }  // K | P | C1 | C2
    // user-layout bounds / refs
    double *dxmin = nullptr, *dxmax = nullptr, *dumin = nullptr, *dumax = nullptr, *dXref = nullptr, *dUref = nullptr;
    // derived
    double *dops = nullptr, *dtables = nullptr;
    bool ops_dirty = true, tables_dirty = true;
    // per-instance state
    double *dx0 = nullptr, *dG = nullptr, *dV = nullptr, *dD = nullptr, *dsolx = nullptr, *dsolu = nullptr;
    int *distats = nullptr;
    int *drefill = nullptr;  // slot refill (layout D): the next-instance counter of a launch (SolveParams::refill_next)
    double *ddstats = nullptr;
    size_t lds_bytes = 0;
    bool tables_in_lds = false;
    bool layout_b = false;  // 4-wave workgroups, V as an HBM ping-pong pair (tinympc_solve_b.hip)
    bool layout_c = false;  // one instance per workgroup, horizon swept in concurrent chunks (tinympc_solve_c.hip)
    // Horizon unrolled at compile time, state in registers, two waves per SIMD (tinympc_solve_d.hip). Wanted for large
    // batches of a shape that is compiled in; each launch still checks that bounds / references are time-invariant and
    // that no family / adaptive rho is active, and otherwise runs the layout-B (or A) kernel on the same HBM state.
    bool layout_d = false;
    bool d_jit = false;     // ... as a run-time specialisation (tinympc_jit.hip) rather than a compiled-in instantiation
    bool d_jit_asked = false;  // the specialiser was asked for the box kernel at setup (its answer may have been a refusal)
    // Large systems, 64 < nx+nu <= 128: tiles of 16 instances on the FP64 matrix cores, state streamed from HBM in the tile's
    // own layout (tinympc_solve_m.hip). The only kernel for these sizes: box path, batched or single, no families /
    // adaptive rho / session.
    bool layout_m = false;
    double dbg_tick[4] = {0.0, 0.0, 0.0, 0.0};  // tinympc_debug_tick_timing
    bool sol_zero_pending = false;  // the device solution is zero by contract (reset_workspace), not yet zeroed: every solve of >= 1 iteration overwrites all of it
    bool sol_ptrs_exported = false;  // tinympc_get_solution_device_ptrs has handed the buffers out: a reset zeroes them eagerly (the caller reads them without a verb)
    bool cold_state = false;  // G, V, D are zero by contract (reset_workspace) but NOT yet zeroed in HBM: see SolveParams::cold
    bool d_varying_jit = false;  // ... and that kernel is a run-time specialisation even if the constant-table one is compiled in
    int d_adapt = -1;       // ... and with adaptive rho
    int d_fam = -1;         // layout D with the cone / linear families (run-time specialised, short horizons): -1 not asked yet, 0 no, 1 yes
    int d_varying = -1;     // layout D with bounds / references that vary over the horizon: -1 not asked yet, 0 no, 1 yes
    // Layout E (tinympc_solve_e.hip, run-time specialised on the families' STRUCTURE): the horizon cut across the wavefronts of a
    // workgroup -- the throughput kernel for the families at horizons layout D cannot hold. Decided per launch
    // (decide_layout_variants): `e_sig` is the structure / table kind the answer `e_ok` belongs to.
    tinympc::FamilyStructure fs;
    std::string e_sig;
    bool e_ok = false;
    int e_chunk_len = 0, e_wpg = 0, e_gpw = 1;
    size_t e_lds = 0;
    // Layout F (tinympc_solve_f.hip): the latency kernel as a run-time specialisation (shape, chunk plan and the families'
    // structure compiled in); decided per launch like layout E
    std::string f_sig;
    bool f_ok = false;
    tinympc::FamilyStructure f_fs;
    signed char f_box_builtin[2] = {-1, -1};  // is the box path's layout F kernel compiled in? [tables constant?]; -1: not asked yet
    unsigned f_box_key = 0;  // decide_layout_f, box path: what the current f_sig was decided for (0: nothing)
    bool specialise_asked = false;  // tinympc_prepare() was called: run-time specialisation is welcome wherever it is faster (decide_layout_f)
    int f_chunk_len = 0, f_chunks = 0, f_wpg = 0;
    size_t f_lds = 0;
    double *dctab_f = nullptr;   // Phi^(S..4S) | Psi^(S..4S) for layout F's chunk length
    int dctab_f_len = 0;
    double *dftab = nullptr;     // layout F: the chunks' input tables T_s | aff for f_chunk_len (k_build_f_input_tables)
    int dftab_cap = 0;           // (slots it was allocated for)
    double *dclock = nullptr;    // (diagnostic build TINY_CLOCK_STAMP only) per-wavefront clock stamps of the last launch
    double *dctab_e = nullptr;   // Phi^S | Psi^S for layout E's chunk length
    int dctab_e_len = 0;         // ... the chunk length it was built for (0: not built)
    // every row of the bounds / references is the same at all knots (what the verbs last received; defaults are)
    bool xmin_const = true, xmax_const = true, umin_const = true, umax_const = true, xref_const = true, uref_const = true;
    bool tables_const() const { return xmin_const && xmax_const && umin_const && umax_const && xref_const && uref_const; }
    bool zero_copy_tick = false;  // this launch reads x0 from / writes u0 to pinned host memory (mpc_step, small batches)
    bool c_tables = false;  // the chunk tables exist (layout C is possible for this shape and not excluded)
    bool fam_c = false;     // the cone / linear families run in the latency kernel's FAM variant
    int chunk_len = 0, chunk_count = 0, chunk_levels = 0;
    size_t lds_bytes_c = 0;
    double *dctab = nullptr;
    double *dV2 = nullptr;
    int n_cone_x = 0, n_cone_u = 0, n_lin_x = 0, n_lin_u = 0;
    // cone / linear families (host copies of what the verbs received; k_admm_solve_fam consumes `dfam`)
    std::vector<int> Acx, qcx, Acu, qcu;
    std::vector<double> cx, cu, Alin_x, blin_x, Alin_u, blin_u;
    double *dfam = nullptr, *dGC = nullptr, *dGL = nullptr, *dLX = nullptr;
    int fam_lin_cap = 0, fam_cone_cap = 0, fam_round_cap = 0;  // capacities `dfam` is laid out for (fam_doubles(), tinympc_device.h)
    size_t fam_alloc_doubles = 0;
    double *h_x0 = nullptr, *h_u0 = nullptr;  // pinned staging for tinympc_mpc_step_batch (and x0 of single-instance handles)
    // Single-instance handles (batch == 1, what the MEX shim creates): set_x0 only fills the pinned h_x0, the next
    // launch reads it from there (and mirrors it into dx0), and the kernels also write solution + statistics into the
    // pinned h_sol -- the reference's per-tick sequence set_x0 / solve / get_solution then costs ONE launch and ONE
    // synchronisation instead of three synchronous copies around the launch.
    double *h_sol = nullptr;           // [X | U | 4 residuals | iter, status | completion flag]
    // Closed-loop session (tinympc_session_begin / _step / _end): the latency kernel stays resident and takes its ticks
    // from this mailbox in pinned memory (layout: SolveParams::mail).
    double *h_mail = nullptr;          // [64] in pinned host memory (the kernel polls across PCIe) ...
    double *h_ans = nullptr;           // [32] pinned: the early answer lines of layout F's resident kernel (SolveParams::host_ans)
    double *d_mail = nullptr;          // ... or, where the host can store into device memory (large BAR), in fine-grained device memory
    double *mailbox() const { return d_mail ? d_mail : h_mail; }  // what the session uses (tinympc_handle.hip: acquire_arenas)
    bool session_active = false;
    bool resident_solves = false;  // tinympc_set_resident: tinympc_solve goes through the resident session kernel where one exists
    bool resident_refused = false; // ... and none does for this configuration (asked once)
    bool session_on_f = false;  // ... and its resident kernel is layout F's (families beyond what the latency kernel's session holds)
    // Taken by everything that writes the mailbox or (re)starts the resident kernel: session_step (for the whole tick), end_session
    // and park_sessions_on_device -- the one place where a thread reaches into a handle it does not own. Lock order: the session
    // registry (tinympc_session.hip) first, then this.
    std::mutex session_mu;
    // references re-sent inside a session that turned out to be the previous ones moved up by one knot (receding horizon):
    // only the new last column travels, with the command (flags 4 / 8); two shifts without a step in between, or any other
    // change, fall back to the full re-read (refs_on_host)
    bool xref_shift = false, uref_shift = false;
    bool session_refs_shifted = false;  // the device copies / tables lag behind the pinned references
    // ONE counter stamps session commands and flag-raising launches alike (both complete by writing their stamp into the
    // same slot of h_sol: a launch after a session must not find its number already there)
    unsigned long long session_seq = 0;  // stamp of the last session command / flag-raising launch
    unsigned long long answered_seq = 0;  // ... of the session tick whose early answer was taken last (its write-out is what host_sol_state 3 waits for)
    bool flag_pending = false;
    // ... and set_x_ref / set_u_ref only fill these pinned copies; the next launch's workgroup rebuilds the
    // reference-dependent table rows from them (refresh_reference_tables): a tick with per-tick references
    // (rocket_landing_constraints.m:86-121) is still one launch and one synchronisation.
    double *h_xref = nullptr, *h_uref = nullptr;
    bool refs_on_host = false;         // the pinned references are newer than dXref / dUref and the tables
    bool x0_on_host = false;           // h_x0 is newer than dx0
    int host_sol_state = 0;            // 0: not valid, 1: a launch that writes it is in flight, 2: valid, 3: a session tick has answered with
                                       //    its first controls; solution + statistics are valid once the stamp behind them reads session_seq
    bool host_path() const { return batch == 1 && h_sol != nullptr && !layout_d && !layout_m; }  // (layout D writes to device memory only)
    bool state_in_global = false;             // horizon too long for LDS: layout-A kernels work on dscratch
    double *dscratch_state = nullptr;
    bool fam_dirty = true;
    // Per-instance references and bounds (tinympc_set_x_ref_batch / _u_ref_batch / _bound_constraints_batch; batched handles): InstState.
    InstState inst;
    bool inst_tables() const { return inst.refs() || inst.bounds || inst.models || inst.fam(); }  // the per-instance table rows are in use
    // rows per instance of the per-instance families store: the row half's count, else the shared rows' (one absent row where there are none)
    int ifam_nl() const {
        const int n = inst.lin ? inst.lin_nl : (n_lin_x > n_lin_u ? n_lin_x : n_lin_u);
        return n > 0 ? n : 1;
    }
    // Goal form (every instance's references AND bounds constant over the horizon): layout D's constant-table kernel carries it, with
    // knot 0's rows per instance; everything else runs on layout A.
    bool iref_goal() const {
        return (inst.x ? inst.x_const : xref_const) && (inst.u ? inst.u_const : uref_const) &&
               (inst.bounds ? inst.bounds_const : xmin_const && xmax_const && umin_const && umax_const);
    }
    // Closed-loop rollout on the device (tinympc_rollout_batch / _device, tinympc_plant_step_batch; k_plant_step, tinympc_rollout.hip).
    // The plant override (tinympc_set_plant_batch): every instance's A_p | B_p | f_p, [batch] blocks, on from the first call (which names
    // the whole batch) until tinympc_clear_plant_batch; the stores stay for the next override. Nothing of the controller reads them.
    bool plant = false;
    double *pA = nullptr, *pB = nullptr, *pf = nullptr;
    // ... and the device buffers the host form logs into and stages its disturbance in: grown on demand (capacities in elements), never
    // shrunk, freed with the handle
    double *rl_x = nullptr, *rl_u = nullptr, *rl_w = nullptr;
    int *rl_it = nullptr, *rl_st = nullptr;
    size_t rl_x_cap = 0, rl_u_cap = 0, rl_w_cap = 0, rl_it_cap = 0, rl_st_cap = 0;
    // Rollout metrics (tinympc_set_rollout_metrics): while on, every plant step runs the scored variant of k_plant_step, which moves
    // every instance's row of 8 doubles on (PlantMetricsParams, tinympc_rollout.h). rm_rows [batch][8] and rm_w (the weights qx | ru)
    // are allocated by the first call and stay until the handle goes; tinympc_clear_rollout_metrics only turns the variant off.
    bool metrics = false;
    double *rm_rows = nullptr, *rm_w = nullptr;
    double rm_tol = 0.0;
    // Rollout noise (tinympc_set_rollout_noise): while on, every plant step runs a noisy variant of k_plant_step (PlantNoiseParams,
    // tinympc_rollout.h) with the tick rn_tick, which then moves on by one. rn_sw / rn_sv: the scales, nx values or [batch][nx]
    // (rn_stride 0 / nx), each allocated for the whole batch by the first call that needs it; rn_w_on / rn_v_on: which family is on.
    // rn_px [batch][nx]: the TRUE state while measurement noise is on (rn_v_on) -- x0 then holds the measurement the next solve reads.
    // Every verb that writes x0 from outside writes the same range of rn_px behind it (mirror_x0_into_px, tinympc_capi.hip).
    bool noise = false, rn_w_on = false, rn_v_on = false;
    double *rn_sw = nullptr, *rn_sv = nullptr, *rn_px = nullptr;
    size_t rn_stride = 0;
    unsigned long long rn_seed = 0, rn_first = 0, rn_tick = 0;
    double *rn_out = nullptr;     // tinympc_get_rollout_noise stages w | v here (grown on demand, capacity in elements)
    size_t rn_out_cap = 0;
    size_t lds_bytes_a = 0;       // layout-A LDS plan (layout B, where it runs, replaces lds_bytes; the families and adaptive rho always use layout A)
    bool tables_in_lds_a = false;

    bool use_layout_d() const {
        return layout_d && (tables_const() || d_varying == 1) && (!families_active() || d_fam == 1) && (!st.adaptive_rho || d_adapt == 1);
    }
    bool use_layout_e() const { return e_ok && !st.adaptive_rho && !use_layout_d(); }
    bool use_layout_f() const { return f_ok && !st.adaptive_rho && !use_layout_d() && !use_layout_e(); }
    bool families_active() const {
        return (st.en_state_soc && n_cone_x > 0) || (st.en_input_soc && n_cone_u > 0) ||
               (st.en_state_linear && n_lin_x > 0) || (st.en_input_linear && n_lin_u > 0);
    }
    void *arena_mail = nullptr;                       // ... and the 4 KB of fine-grained device memory that travel with them (the session's mailbox, d_mail)
    void *arena_dev = nullptr, *arena_pin = nullptr;  // the setup arenas (ArenaPlan below; pooled per device, tinympc_handle.hip)
    size_t arena_dev_bytes = 0, arena_pin_bytes = 0;
    std::vector<void *> allocs;       // hipMalloc blocks dalloc() added after setup
    std::vector<void *> host_allocs;  // hipHostMalloc blocks added after setup (staging of mpc_step_batch on batched handles)
    double *h_stage = nullptr;        // pinned staging of the problem data (setup's one upload); layout = the device arena's upload block
    double setup_us[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // tinympc_debug_setup_timing: host microseconds of setup's phases

    size_t X() const { return (size_t)nx * N; }
    size_t U() const { return (size_t)nu * (N - 1); }
    size_t state_doubles() const { return layout_m ? tinympc::solve_m_state_doubles(nx, nu, N, groups) : (size_t)groups * (N + 1) * 64; }  // G; row N: per-lane dummy slot
    size_t v_doubles() const { return layout_m ? tinympc::solve_m_state_doubles(nx, nu, N, groups) : (size_t)groups * tinympc::v_rows(N) * 64; }     // V (and V2)
    size_t d_doubles() const { return layout_m ? tinympc::solve_m_state_doubles(nx, nu, N, groups) : (size_t)groups * (N - 1) * IPW * nu; }
};

namespace tinympc {
namespace host {

void park_sessions_on_device(int device, const tinympc_solver *except);  // (tinympc_session.hip; described below)

// One block of device memory and one block of pinned host memory per handle (round 5): every array whose size is known at setup is
// carved out of them -- tinympc_setup_batch used to make ~45 hipMalloc and 5 hipHostMalloc calls (5.9 ms for a quadrotor, twelve
// times the reference's whole tiny_setup). ArenaPlan collects (slot, offset) pairs in a first pass, the block is allocated once,
// bind() writes the pointers. 256-byte alignment: every array starts on its own pair of 128-byte lines.
struct ArenaPlan {
    struct Item { void **slot; size_t offset; };
    std::vector<Item> items;
    size_t total = 0;
    size_t mark() { total = (total + 255) & ~(size_t)255; return total; }
    template <typename T>
    void add(T **slot, size_t count) {
        mark();
        items.push_back({reinterpret_cast<void **>(slot), total});
        total += sizeof(T) * (count ? count : 1);
    }
    void bind(void *base) const {
        for (const Item &it : items) *it.slot = static_cast<char *>(base) + it.offset;
    }
};

// Arrays whose size depends on what the verbs receive AFTER setup (the families' description and duals, a longer layout-F chunk,
// the HBM working copy of a long horizon on layout M): their own hipMalloc, at the launch that first needs them. hipMalloc
// synchronises the device, so resident session kernels of OTHER handles are sent home first (as setup and destroy do) -- it would
// otherwise stall until their 2 s idle time-out. Not from inside this handle's own session tick (session_mu is held there and the
// registry lock comes first in the lock order): a session's kernel was launched once by session_begin, everything it needs exists.
template <typename T>
int dalloc(tinympc_solver *s, T **p, size_t count) {
    if (!s->session_active) park_sessions_on_device(s->device, s);
    void *q = nullptr;
    hipError_t e = hipMalloc(&q, sizeof(T) * (count ? count : 1));
    if (e != hipSuccess) return fail(TINYMPC_ERR_ALLOC, "hipMalloc(%zu bytes) failed: %s", sizeof(T) * count, hipGetErrorString(e));
    s->allocs.push_back(q);
    *p = static_cast<T *>(q);
    return TINYMPC_OK;
}

// ---- tinympc_handle.hip
int acquire_arenas(tinympc_solver *s, size_t dev_bytes, size_t pin_bytes, bool want_mailbox);  // -> s->arena_dev / arena_pin (from the device's pool when one fits)
int acquire_stream_kit(tinympc_solver *s);  // stream + event pair from the device's pool (created when the pool is empty)
int bind_device(tinympc_solver *s);   // every verb that touches the device passes through here first (ends an open session)
bool queues_may_be_shared(int device);  // the library's streams on `device` may share hardware queues (more than GPU_MAX_HW_QUEUES)
bool rows_constant(const double *m, int rows, int cols);
int upload(tinympc_solver *s, double *dst, const double *src, size_t count);
int download(tinympc_solver *s, void *dst, const void *src, size_t bytes);
int fill_host_upload(tinympc_solver *s, double *dst, size_t count, double value);
int check_handle(const tinympc_solver *s);
int run_precompute(tinympc_solver *s);
int flush_host_refs(tinympc_solver *s);
int refresh_derived(tinympc_solver *s);
FamilyStructure family_structure(const tinympc_solver *s, double *mu = nullptr);
int refresh_families(tinympc_solver *s);
int refresh_inst_families(tinympc_solver *s);  // the per-instance families store: its copy of the shared rows (slope half alone) and its slope vectors
int refresh_inst_tables(tinympc_solver *s);  // the per-instance table rows of the instances whose references / bounds / models changed
int alloc_inst_rows(tinympc_solver *s, bool bounds);  // the table rows themselves (allocated by the first per-instance verb that needs them)
void destroy(tinympc_solver *s);

// ---- tinympc_plan.hip: the kernel of a launch, decided in ONE place
enum class KernelId { M, D_COMPILED, D_JIT, E, F, C, FAM_A, ADAPT_A, B, A };
struct LaunchPlan {
    KernelId kernel = KernelId::A;
    char layout = 'A';                       // what tinympc_get_layout reports
    bool families = false, adaptive = false;  // variant bits of the launch
    bool inst_refs = false;                  // ... per-instance references (layout A's InstRefs variant) or bounds (see inst_bounds)
    bool inst_bounds = false;                // ... per-instance bounds (layout A's InstBounds variant)
    bool inst_models = false;                // ... per-instance models (layout A's InstModels variant; inst_refs and inst_bounds are set with it)
    bool inst_lin = false;                   // ... per-instance linear rows (layout A's InstFamilies variant, or layout D's ILIN form: D_JIT; inst_refs and inst_bounds are set with it)
    bool inst_kbnd = false;                  // ... bounds per knot on layout D's IKBND form (D_JIT; inst_refs is set with it; inst_traj beside it: IKBND with ITRAJ)
    bool inst_traj = false;                  // ... per-instance trajectories / tracks on layout D's ITRAJ form (D_JIT; inst_refs is set with it; beside inst_lin: the families' form on them)
    bool jit = false;                        // a run-time specialisation (tinympc_jit.hip) rather than a compiled-in kernel
    bool host_exchange = false;              // the kernel serves the pinned-host paths (x0 in, solution / completion stamp out)
    int workgroups = 0;
    size_t lds_bytes = 0;
    bool tables_in_lds = false;
};
LaunchPlan current_plan(const tinympc_solver *s);  // from what has been decided so far (compiles nothing)
int resolve_plan(tinympc_solver *s);               // decide (and, where needed, specialise) the variants of the current configuration
int check_launch(const tinympc_solver *s, const LaunchPlan &pl);  // what launch() refuses for plan `pl`, with its message; queues and changes nothing
int launch(tinympc_solver *s, bool timed);

// ---- tinympc_session.hip
int end_session(tinympc_solver *s);
int wait_session_solution(tinympc_solver *s);  // host_sol_state 3 -> 2: spins on the completion stamp of the last session tick
// Resident session kernels of OTHER handles on `device` are sent home before anything that synchronises the device (hipMalloc /
// hipFree in setup and teardown): such a call would otherwise stall until the spinning kernel's idle time-out (2 s). Their
// sessions stay open: the next session_step finds the kernel gone and starts it again (its restart path).
void park_sessions_on_device(int device, const tinympc_solver *except);
// Writes the zeros of a pending cold start into G, V, D (for a kernel that loads its state from HBM whatever its value).
int materialize_cold_state(tinympc_solver *s);
// ... and of a pending zero solution into sol_x / sol_u (before anything reads them that no solve has written since the reset).
int materialize_zero_solution(tinympc_solver *s);

}  // namespace host
}  // namespace tinympc
