// tinympc_plan.hip -- WHICH kernel a launch runs, and the launch. Nine kernel families (tinympc_device.h) x (compiled in | run-time
// specialised) x (constant | per-knot tables) x (box path | cone / linear families | adaptive rho): the choice is made in ONE
// function, current_plan(), from the handle's capabilities (what setup found possible for the shape) and the variants decided
// for the CURRENT configuration (resolve_plan(): may specialise a kernel, seconds the first time). launch(), the launch geometry
// of tinympc_get_launch_info, tinympc_get_layout and tinympc_get_jit_info all read that one LaunchPlan.
#include <cstring>
#include "tinympc_handle.h"

using namespace tinympc;
using namespace tinympc::host;

namespace {

// Single-instance launches of the latency kernel end by writing a sequence number behind the solution in pinned host
// memory; tinympc_synchronize polls it (a few hundred nanoseconds after the kernel's last store) instead of sleeping in
// hipStreamSynchronize (whose wake-up costs several microseconds of a ~25 us tick).
void arm_completion_flag(tinympc_solver *s, SolveParams &p) {
    if (!p.host_sol) return;
    s->session_seq += 1;
    p.host_seq = (double)s->session_seq;
    s->flag_pending = true;
}

// Layout D's variants beyond the constant-table box path are decided when first needed (they may have to be specialised,
// which takes seconds): time-varying tables and the cone / linear families. Called by everything that asks use_layout_d()
// before a launch, so that the answer does not change between that question and the launch itself.
void decide_layout_d_variants(tinympc_solver *s) {
    if (!s->layout_d) return;
    if (s->d_varying < 0 && !s->tables_const()) {
        // is there a kernel for per-knot tables (compiled in -- 16-lane form only -- or specialised now)? Otherwise these launches
        // run on layout B / A, as before.
        if (s->W == 16 && !s->d_jit && solve_d_supported(s->nx, s->nu, s->N, false)) {
            s->d_varying = 1;
        } else {
            s->d_varying_jit = solve_jit_supported(s->W, s->nx, s->nu, s->N, false);
            s->d_varying = s->d_varying_jit ? 1 : 0;
        }
    }
    if (s->st.adaptive_rho && !s->families_active())
        s->d_adapt = (s->W == 16 && solve_jit_supported(s->W, s->nx, s->nu, s->N, s->tables_const(), false, true)) ? 1 : 0;
    if (s->families_active() && !s->st.adaptive_rho) {
        // families: a run-time specialisation (16-lane form, horizons whose five register pairs per knot fit)? Asked every
        // time -- the answer is cached inside -- because it also depends on the tables' kind.
        // (cones that share rows need the round-by-round projection, which layout D's families variant and the latency kernel
        // do not have: layout E or k_admm_solve_fam run those)
        const FamilyStructure fsd = family_structure(s);
        // Round 4: at these horizons layout E has an UNCUT form (one wavefront per group, the families one knot per lane) that does in
        // ~200 instructions per iteration what this variant pays in every slot -- it takes precedence where it builds (TINYMPC_LAYOUT=D
        // keeps the variant for the tests and A/B runs).
        bool e_uncut = false;
        const char *env = getenv("TINYMPC_LAYOUT");
        if (s->W == 16 && s->batch > 1 && s->N - 1 <= 31 && !(env && (env[0] == 'D' || env[0] == 'd'))) {
            int wpg = 0;
            e_uncut = solve_e_plan(s->nx, s->nu, s->N, s->tables_const(), true, fsd, nullptr, &wpg, nullptr, nullptr) && wpg == 1 &&
                      solve_e_supported(s->nx, s->nu, s->N, s->tables_const(), true, fsd);
        }
        if (s->W == 16)
            s->d_fam = (!e_uncut && fsd.nround <= 1 && !fsd.beyond_generic() && solve_jit_supported(s->W, s->nx, s->nu, s->N, s->tables_const(), true)) ? 1 : 0;
        else  // (round 5) wide systems: the families streamed from HBM next to the register-resident box sweeps; rounds are walked there
            s->d_fam = (!s->layout_m && !fsd.beyond_generic() && fsd.nround <= MAX_ROUNDS && solve_jit_supported(s->W, s->nx, s->nu, s->N, s->tables_const(), true)) ? 1 : 0;
    }
}

// Layout E for the families where layout D has no kernel (long horizons): asked whenever the structure of the families or the
// kind of the tables changed (the kernel is specialised on both; compiling takes seconds the first time, the answer is cached
// inside tinympc_jit.hip). TINYMPC_LAYOUT=E forces it at any batch size (tests), any other value excludes it.
int decide_layout_e(tinympc_solver *s) {
    const bool fam = s->families_active();
    // (single-instance handles exchange x0 / the solution through pinned host memory, which only the latency kernel serves)
    const bool possible = s->W == 16 && !s->layout_m && !s->st.adaptive_rho && s->batch > 1;
    // families: wherever layout D has no kernel; box path: horizons for which the specialiser has no layout-D kernel at all (no plan,
    // or a plan whose code object spilled) -- long horizons, where layouts B / A are left with one or two wavefronts per CU
    bool want = possible && !s->use_layout_d() &&
                (fam ? s->batch >= kLayoutEBatchMin : (s->d_jit_asked && !s->layout_d && s->batch > kLayoutCBatchMax && s->N >= 26));
    if (const char *env = getenv("TINYMPC_LAYOUT")) want = (env[0] == 'E' || env[0] == 'e') && possible;
    if (!want) {
        s->e_ok = false;
        s->e_sig.clear();
        return TINYMPC_OK;
    }
    const FamilyStructure fs = fam ? family_structure(s) : FamilyStructure();
    std::string sig = s->tables_const() ? "ct|" : "var|";
    for (int c = 0; c < fs.ncone; ++c) sig += std::to_string(fs.cone[c][0]) + "," + std::to_string(fs.cone[c][1]) + "," + std::to_string(fs.cone[c][2]) + ";";
    sig += "|" + std::to_string(fs.nlx) + "," + std::to_string(fs.nlu) + (fam ? "|fam" : "|box");
    sig += solve_jit_enabled() ? "|jit" : "|nojit";  // (TINYMPC_JIT=0 switches the specialised kernels off from the next launch on)
    if (sig == s->e_sig) return TINYMPC_OK;
    s->e_sig = sig;
    s->fs = fs;
    s->e_ok = solve_e_supported(s->nx, s->nu, s->N, s->tables_const(), fam, fs) &&
              solve_e_plan(s->nx, s->nu, s->N, s->tables_const(), fam, fs, &s->e_chunk_len, &s->e_wpg, &s->e_lds, &s->e_gpw);
    if (s->e_ok && !s->dctab_e) {
        int rc = dalloc(s, &s->dctab_e, chunk_table_doubles(s->nx, 1));
        if (rc) return rc;
    }
    return TINYMPC_OK;
}

// Layout F for what the latency kernel (layout C) serves: single solves and small batches. The kernel is specialised on the
// shape, the kind of the tables and the structure of the families, so it is asked whenever one of them changed (seconds the
// first time; cached inside tinympc_jit.hip). TINYMPC_LAYOUT=F forces it at any batch size (tests), any other value excludes it.
int decide_layout_f(tinympc_solver *s) {
    const bool fam = s->families_active();
    const bool possible = s->W == 16 && !s->layout_m && !s->st.adaptive_rho && (!s->session_active || s->session_on_f) && s->N >= 6;
    // Default: the families at small batches -- rocket landing N=100, one instance: 4.5 us per iteration against 6.55 on the
    // round-1 latency kernel
    // (a configuration beyond what the generic kernels hold -- more than MAX_LIN_ROWS rows, MAX_CONES cones, MAX_ROUNDS rounds -- has
    // no other kernel at these batch sizes)
    bool want = possible && fam && !s->use_layout_d() && !s->use_layout_e() && s->batch < kLayoutEBatchMin &&
                (s->fam_c || family_structure(s).beyond_generic());
    // ... and (round 4) the box path wherever the latency kernel would run: layout F is ahead on every shape measured
    // (tools/single_cf_probe.py, microseconds per iteration, one instance: quadrotor N=10 / 20 / 50 / 100 1.81 / 2.24 / 2.73 / 4.07
    // against 2.45 / 2.63 / 2.90 / 4.33, cartpole N=20 1.60 against 2.13) and has had the resident session since this round. It is
    // a specialisation, though: a first setup of a new shape must not cost seconds behind the caller's back, so it is taken where it
    // costs nothing -- the configurations compiled into the library (BASELINE configs 2 and 3) -- or where the caller asked for the
    // specialised kernels with tinympc_prepare() (the real-time workflow of INTEGRATION.md); otherwise layout C, which needs none.
    bool box_f = possible && !fam && s->layout_c && !s->use_layout_d() && !s->use_layout_e() && solve_jit_enabled();
    if (box_f && !s->specialise_asked) {  // (asked once per handle and kind of tables: this runs in front of every launch)
        signed char &known = s->f_box_builtin[s->tables_const() ? 1 : 0];
        if (known < 0) known = solve_f_builtin(s->nx, s->nu, s->N, s->tables_const(), false, FamilyStructure(), false) ? 1 : 0;
        box_f = known == 1;
    }
    want = want || box_f;
    if (const char *env = getenv("TINYMPC_LAYOUT")) want = (env[0] == 'F' || env[0] == 'f') && possible;
    if (!want) {
        s->f_ok = false;
        s->f_sig.clear();
        s->f_box_key = 0;
        return TINYMPC_OK;
    }
    // (the box path decides in front of every closed-loop tick: a small integer instead of the signature string below)
    const unsigned box_key = fam ? 0u : (8u | (s->tables_const() ? 1u : 0u) | (solve_jit_enabled() ? 2u : 0u));
    if (!fam && box_key == s->f_box_key && !s->f_sig.empty()) return TINYMPC_OK;
    s->f_box_key = box_key;
    const FamilyStructure fs = fam ? family_structure(s) : FamilyStructure();
    std::string sig = s->tables_const() ? "ct|" : "var|";
    for (int c = 0; c < fs.ncone; ++c) sig += std::to_string(fs.cone[c][0]) + "," + std::to_string(fs.cone[c][1]) + "," + std::to_string(fs.cone[c][2]) + ";";
    sig += "|" + std::to_string(fs.nlx) + "," + std::to_string(fs.nlu) + (fam ? "|fam" : "|box");
    sig += solve_jit_enabled() ? "|jit" : "|nojit";
    if (sig == s->f_sig) return TINYMPC_OK;
    s->f_sig = sig;
    s->f_fs = fs;
    s->f_ok = solve_f_supported(s->nx, s->nu, s->N, s->tables_const(), fam, fs) &&
              solve_f_plan(s->nx, s->nu, s->N, s->tables_const(), fam, fs, &s->f_chunk_len, &s->f_chunks, &s->f_wpg, &s->f_lds);
    if (s->f_ok && !s->dctab_f) {
        int rc = dalloc(s, &s->dctab_f, chunk_table_doubles(s->nx, 4));
        if (rc) return rc;
    }
    return TINYMPC_OK;
}

// (per-launch pieces of the plan's run-time specialised kernels)
bool d_is_jit(const tinympc_solver *s, bool fam, bool adaptive) {
    return s->d_jit || fam || adaptive || (!s->tables_const() && s->d_varying_jit);
}

// Per-instance models on layout D: opt-in (tinympc_prepare -- without it the mode stays on layout A, which needs no specialisation),
// where the handle runs layout D, 16 lanes per instance (wider operators do not fit a wavefront's LDS share), references and bounds
// constant over the horizon, box path. Whether the kernel exists is inst.d_models (resolve_plan).
bool models_want_d(const tinympc_solver *s) {
    return s->inst.models && !s->inst.fam() && s->specialise_asked && s->layout_d && !s->layout_m && s->W == 16 && s->iref_goal() && !s->families_active() &&
           !s->st.adaptive_rho;
}

// Per-instance trajectories and tracks on layout D: opt-in like the models' form (tinympc_prepare -- without it they stay on layout A, which
// needs no specialisation), where the handle runs layout D, 16 lanes per instance, at least one half of the references is a per-instance
// trajectory or track (where every half is constant over the horizon the goal form keeps precedence), bounds constant over the horizon
// (shared or per instance), box path, the shared model and rho. Whether the kernel exists -- the horizon's rows fit a wavefront's LDS
// share -- is inst.d_traj (resolve_plan).
bool traj_wants_d(const tinympc_solver *s) {
    const InstState &in = s->inst;
    const bool traj = (in.x && !in.x_const) || (in.u && !in.u_const);
    const bool bounds_const = in.bounds ? in.bounds_const : s->xmin_const && s->xmax_const && s->umin_const && s->umax_const;
    return traj && bounds_const && !in.models && !in.fam() && s->specialise_asked && s->layout_d && !s->layout_m && s->W == 16 && !s->families_active() &&
           !s->st.adaptive_rho;
}

// Box bounds that vary over the horizon on layout D: opt-in like the trajectory form (tinympc_prepare), where the handle runs layout D, 16
// lanes per instance, box path, the shared model and rho, and the bounds are per instance and per knot (tinympc_set_bound_constraints_batch
// with a column per knot) or shared per-knot bounds beside per-instance trajectories / tracks. Every reference half is constant over the
// horizon (shared or per instance) or a per-instance trajectory / track (kbnd_traj: the form then has ITRAJ beside IKBND) -- a SHARED
// trajectory, tinympc_set_x_ref / _set_u_ref, keeps the mode on layout A. Whether the kernel exists -- the horizon's clamp rows fit a
// wavefront's LDS share -- is inst.d_kbnd for the variant inst.d_kbnd_traj (resolve_plan).
bool kbnd_traj(const tinympc_solver *s) { return (s->inst.x && !s->inst.x_const) || (s->inst.u && !s->inst.u_const); }
bool kbnd_wants_d(const tinympc_solver *s) {
    const InstState &in = s->inst;
    const bool shared_const = s->xmin_const && s->xmax_const && s->umin_const && s->umax_const;
    const bool per_knot = in.bounds ? !in.bounds_const : !shared_const && kbnd_traj(s);
    return per_knot && (in.x || s->xref_const) && (in.u || s->uref_const) && !in.models && !in.fam() && s->specialise_asked && s->layout_d && !s->layout_m && s->W == 16 &&
           !s->families_active() && !s->st.adaptive_rho;
}
bool kbnd_on_d(const tinympc_solver *s) { return kbnd_wants_d(s) && s->inst.d_kbnd == 1 && s->inst.d_kbnd_traj == kbnd_traj(s); }

// Per-instance linear rows (tinympc_set_linear_constraints_batch): layout A's InstFamilies variant, or layout D's ILIN form (below). What
// neither can carry is refused at the launch (lin_refusal), never solved with shared rows.
bool lin_runs(const tinympc_solver *s) {
    return s->inst.fam() && !s->layout_m && !s->inst.models && !s->st.adaptive_rho && !family_structure(s).beyond_generic();
}
// ... on layout D: opt-in like the models' form (tinympc_prepare -- without it the mode stays on layout A, which needs no specialisation),
// where the handle runs layout D, 16 lanes per instance, bounds constant over the horizon (shared or per instance: no per-knot bounds),
// every half of the references constant over the horizon (shared or per instance) or a per-instance trajectory / track (lin_d_traj:
// the form then reads its linref rows per wavefront, ITRAJ -- a SHARED trajectory, tinympc_set_x_ref / _set_u_ref, keeps the mode on
// layout A), and a cone structure layout D's shared families kernel takes (decide_layout_d_variants: no rounds of overlapping cones).
// Whether the kernel exists for the mode's row count is inst.d_lin (resolve_plan).
// Rows per knot (tinympc_set_linear_constraints_knots_batch) take the same way: the form's per-knot variant (lin_d_knots), whose
// per-wavefront plan holds N slots of rows -- where it does not fit the mode stays on layout A's InstFamiliesKnots variant.
int lin_d_knots(const tinympc_solver *s) { return s->inst.lin ? s->inst.lin_knots : 0; }
bool lin_d_traj(const tinympc_solver *s) { return (s->inst.x && !s->inst.x_const) || (s->inst.u && !s->inst.u_const); }
// (references and bounds as the form takes them: iref_goal() with "constant" relaxed to "or a per-instance trajectory" on each reference half)
bool lin_refs_fit_d(const tinympc_solver *s) {
    const InstState &in = s->inst;
    return (in.x || s->xref_const) && (in.u || s->uref_const) && (in.bounds ? in.bounds_const : s->xmin_const && s->xmax_const && s->umin_const && s->umax_const);
}
bool lin_wants_d(const tinympc_solver *s) {
    return lin_runs(s) && s->specialise_asked && s->layout_d && s->W == 16 && lin_refs_fit_d(s) && family_structure(s).nround <= 1;
}
// (the answer inst.d_lin is the one for this mode's row count, slopes, knots and trajectories)
bool lin_d_answer_current(const tinympc_solver *s) {
    return s->inst.d_lin_nl == s->ifam_nl() && s->inst.d_lin_cones == s->inst.cones && s->inst.d_lin_knots == lin_d_knots(s) && s->inst.d_lin_traj == lin_d_traj(s);
}
bool lin_on_d(const tinympc_solver *s) { return lin_wants_d(s) && s->inst.d_lin == 1 && lin_d_answer_current(s); }

}  // namespace

namespace tinympc {
namespace host {

// The one place where the kernel of a launch is chosen. Order of preference per variant:
//   large systems                      M
//   adaptive rho                       D (run-time specialised, rho per lane)  >  k_admm_solve_adapt on layout A's plan
//   cone / linear families             D (N <= 22)  >  F (small batches)  >  E (batches)  >  C<FAM> (disjoint cones only)  >  k_admm_solve_fam
//   box path                           E (only where D has no kernel)  >  D  >  F (on request)  >  C (small batches)  >  B  >  A
//   per-instance references / bounds   D's goal form  >  A (box path only: with the families, adaptive rho or layout M, launch() refuses)
//   per-instance models                D's model form (only after tinympc_prepare: 16 lanes, references and bounds constant over the horizon,
//                                      a horizon its per-wavefront operator plan holds)  >  A (the same refusals)
//                                      (the mode of tinympc_set_model_batch AND tinympc_set_rho_batch: one form, rho always read per instance)
//   bounds per knot, per instance      D's IKBND form (only after tinympc_prepare: 16 lanes, box path, shared model and rho; bounds per instance and
//                                      knot, or shared per-knot bounds beside per-instance trajectories / tracks; every reference half constant
//                                      or a per-instance trajectory / track -- then IKBND with ITRAJ; a horizon whose clamp rows its
//                                      per-wavefront plan holds: quadrotor N <= 33, N <= 22 beside trajectories)  >  A's InstBounds variant
//   per-instance linear rows           D's ILIN form (only after tinympc_prepare: 16 lanes, bounds constant over the horizon, every reference half
//                                      constant over the horizon or a per-instance trajectory / track -- then ILIN with ITRAJ, the wavefront's
//                                      own linref rows behind its linear rows; a SHARED trajectory stays on layout A --, cones
//                                      without rounds, a horizon and row count its per-wavefront plan holds)  >  A's InstFamilies variant,
//                                      (rows per knot: the form's per-knot variant, N slots of rows per wavefront -- one row up to N=22, two up
//                                      to N=12, three up to N=8; beside trajectories N=17, 10, 7 for the quadrotor  >  A's InstFamiliesKnots variant),
//                                      whatever else is per instance (references, bounds) or shared (cones); with
//                                      per-instance models / rho, adaptive rho, layout M or a cone structure beyond the generic kernels, launch() refuses
LaunchPlan current_plan(const tinympc_solver *s) {
    LaunchPlan pl;
    const bool fam = s->families_active(), adaptive = s->st.adaptive_rho != 0, d = s->use_layout_d();
    pl.families = fam;
    pl.adaptive = adaptive;
    if (lin_runs(s)) {
        pl.kernel = lin_on_d(s) ? KernelId::D_JIT : KernelId::A;
        pl.inst_lin = pl.inst_refs = pl.inst_bounds = true;  // (both kernels always run on per-instance reference and clamp rows)
        pl.inst_traj = pl.kernel == KernelId::D_JIT && lin_d_traj(s);  // (the form on the wavefront's own linref rows)
    } else if (s->inst_tables() && !s->inst.fam() && !s->layout_m && !fam && !adaptive) {
        // goals, where the handle runs layout D: its constant-table kernel (compiled in for the 16-lane shapes that are, run-time
        // specialised otherwise -- wide systems included); trajectories, and goals without such a kernel: layout A. "Goal" means that
        // references AND bounds are constant over the horizon, each per instance or shared
        // models: layout A's InstModels variant, or -- where the caller asked for specialised kernels -- layout D's model form (the goal
        // form with every wavefront's four operator blocks in its own LDS region; compiled in or run-time specialised: KernelId::D_JIT)
        const bool goal = s->layout_d && s->iref_goal() && !s->inst.models;
        const bool d_models = models_want_d(s) && s->inst.d_models == 1;
        // trajectories and tracks: layout A's InstRefs / InstBounds variants, or -- under the same opt-in -- layout D's trajectory form (the
        // goal form with every wavefront's own linref rows in its LDS region: KernelId::D_JIT)
        pl.inst_traj = !goal && traj_wants_d(s) && s->inst.d_traj == 1;
        // bounds per knot: layout A's InstBounds variant (or its shared tables), or -- under the same opt-in -- layout D's per-knot bounds form
        // (the goal form with every wavefront's own clamp rows in its LDS region, and its linref rows beside trajectories: KernelId::D_JIT)
        pl.inst_kbnd = !goal && kbnd_on_d(s);
        if (pl.inst_kbnd) pl.inst_traj = kbnd_traj(s);
        pl.kernel = (goal && !s->d_jit && s->W == 16 && solve_d_supported(s->nx, s->nu, s->N, true)) ? KernelId::D_COMPILED
                    : ((goal && s->inst.d_goal == 1) || d_models || pl.inst_traj || pl.inst_kbnd) ? KernelId::D_JIT : KernelId::A;
        pl.inst_refs = true;
        pl.inst_models = s->inst.models;
        pl.inst_bounds = s->inst.bounds || pl.inst_models;  // (the models' variant always runs on per-instance clamp rows)
    } else if (s->layout_m) pl.kernel = KernelId::M;
    else if (adaptive) pl.kernel = d ? KernelId::D_JIT : KernelId::ADAPT_A;
    else if (fam)
        pl.kernel = d ? KernelId::D_JIT : s->use_layout_f() ? KernelId::F : s->use_layout_e() ? KernelId::E
                    : (s->fam_c && family_structure(s).nround <= 1) ? KernelId::C : KernelId::FAM_A;
    else
        pl.kernel = s->use_layout_e() ? KernelId::E : d ? (d_is_jit(s, false, false) ? KernelId::D_JIT : KernelId::D_COMPILED)
                    : s->use_layout_f() ? KernelId::F : s->layout_c ? KernelId::C : s->layout_b ? KernelId::B : KernelId::A;
    const bool d_goal = pl.inst_refs && (pl.kernel == KernelId::D_COMPILED || pl.kernel == KernelId::D_JIT);
    const bool ct = s->tables_const() || d_goal;  // (the goal form: constant tables)
    switch (pl.kernel) {
        case KernelId::M:
            pl.layout = 'M';
            pl.workgroups = s->groups;
            pl.lds_bytes = 0;  // (static LDS: see the kernel)
            break;
        case KernelId::D_JIT: {
            pl.layout = 'D';
            pl.jit = true;
            const int ilin = pl.inst_lin ? s->ifam_nl() : 0;  // (the ILIN form: the families' kernel whichever sides are enabled)
            pl.workgroups = solve_jit_workgroups(s->W, s->nx, s->nu, s->N, ct, s->groups, fam || ilin, adaptive, pl.inst_refs, pl.inst_models, ilin, ilin && s->inst.cones,
                                                 ilin ? lin_d_knots(s) : 0, pl.inst_traj, pl.inst_kbnd);
            pl.lds_bytes = solve_jit_lds_bytes(s->W, s->nx, s->nu, s->N, ct, fam || ilin, adaptive, pl.inst_refs, pl.inst_models, ilin, ilin && s->inst.cones, ilin ? lin_d_knots(s) : 0,
                                               pl.inst_traj, pl.inst_kbnd);
            break;
        }
        case KernelId::D_COMPILED:
            pl.layout = 'D';
            pl.host_exchange = s->W == 16 && !pl.inst_refs;  // (the compiled-in 16-lane shapes have a variant that reads x0 from / writes the first controls to pinned host memory)
            pl.workgroups = s->W == 64 ? solve_dx_workgroups(s->nu, s->N, s->groups) : s->W == 32 ? solve_dw_workgroups(s->nu, s->N, s->groups)
                                                                                                   : solve_d_workgroups(s->nu, s->N, ct, s->groups);
            pl.lds_bytes = s->W == 64 ? solve_dx_lds_bytes(s->nu, s->N) : s->W == 32 ? solve_dw_lds_bytes(s->nu, s->N) : solve_d_lds_bytes(s->nu, s->N, ct);
            break;
        case KernelId::E:
            pl.layout = 'E';
            pl.jit = true;
            pl.workgroups = (s->groups + s->e_gpw - 1) / s->e_gpw;
            pl.lds_bytes = s->e_lds;
            break;
        case KernelId::F:
            pl.layout = 'F';
            pl.jit = true;
            pl.host_exchange = true;
            pl.workgroups = s->batch;
            pl.lds_bytes = s->f_lds;
            break;
        case KernelId::C:
            pl.layout = 'C';
            pl.host_exchange = true;
            pl.workgroups = s->batch;
            pl.lds_bytes = s->lds_bytes_c;
            break;
        case KernelId::B:
            pl.layout = 'B';
            pl.host_exchange = true;
            pl.workgroups = (s->groups + WAVES_PER_GROUP_B - 1) / WAVES_PER_GROUP_B;
            pl.lds_bytes = s->lds_bytes;
            pl.tables_in_lds = s->tables_in_lds;
            break;
        case KernelId::A:
        case KernelId::FAM_A:
        case KernelId::ADAPT_A:  // (layout A's own plan: A itself runs only where layout B does not)
            pl.layout = 'A';
            pl.host_exchange = true;
            pl.workgroups = s->groups;
            pl.lds_bytes = s->lds_bytes_a;
            pl.tables_in_lds = s->tables_in_lds_a;
            break;
    }
    return pl;
}

int resolve_plan(tinympc_solver *s) {
    int rc;
    if (s->inst_tables()) {  // layout A or D's goal form, or a refusal: only the goal form's specialisation to decide
        int &known = s->inst.d_goal;
        if (known < 0 && !s->inst.fam() && s->layout_d && s->iref_goal() && !s->inst.models && !(s->W == 16 && !s->d_jit && solve_d_supported(s->nx, s->nu, s->N, true)) &&
            !s->families_active() && !s->st.adaptive_rho)
            known = solve_jit_supported(s->W, s->nx, s->nu, s->N, true, false, false, true) ? 1 : 0;
        // ... and the model form's (compiled in for the quadrotor N=50, specialised now otherwise; a refusal leaves the mode on layout A)
        if (s->inst.d_models < 0 && models_want_d(s))
            s->inst.d_models = solve_jit_supported(s->W, s->nx, s->nu, s->N, true, false, false, false, true) ? 1 : 0;
        // ... and the trajectory form's (compiled in for the quadrotor N=50, specialised now otherwise; a horizon whose rows fit no plan, or
        // a refusal, leaves trajectories and tracks on layout A)
        if (s->inst.d_traj < 0 && traj_wants_d(s))
            s->inst.d_traj = solve_jit_supported(s->W, s->nx, s->nu, s->N, true, false, false, true, false, 0, false, 0, true) ? 1 : 0;
        // ... and the per-knot bounds form's, for the mode's ITRAJ variant (compiled in for the quadrotor N=20 with trajectories, specialised now
        // otherwise). A horizon whose rows fit no plan is no refusal (2); the other variant is another specialisation: asked again.
        if (kbnd_wants_d(s)) {
            InstState &in = s->inst;
            const bool tr = kbnd_traj(s);
            if (in.d_kbnd >= 0 && in.d_kbnd_traj != tr) in.d_kbnd = -1;
            if (in.d_kbnd < 0) {
                in.d_kbnd_traj = tr;
                in.d_kbnd = !solve_jit_planned(s->W, s->nx, s->nu, s->N, true, false, false, false, 0, 0, tr, true) ? 2
                            : solve_jit_supported(s->W, s->nx, s->nu, s->N, true, false, false, true, false, 0, false, 0, tr, true) ? 1 : 0;
            }
            if (in.d_kbnd == 1 && !in.bnd_always) {  // (the form reads layout A's clamp rows whether the bounds are per instance or shared)
                if ((rc = alloc_inst_rows(s, true))) return rc;
                in.bnd_always = true;
                in.mark(0, s->batch);
            }
        }
        // ... and the linear-row form's, for the mode's row count (compiled in for the quadrotor N=20 with one row, specialised now
        // otherwise; a refusal leaves the mode on layout A). Another count is another specialisation: asked again -- and so is the other
        // of rows constant over the horizon and rows per knot (compiled in for the same quadrotor with one row).
        // ... and of references constant over the horizon and per-instance trajectories / tracks (compiled in for the same quadrotor with
        // one row): the trajectory bit is one more part of the answer.
        if (s->inst.fam() && !lin_d_answer_current(s)) s->inst.d_lin = -1;
        if (s->inst.d_lin < 0 && lin_wants_d(s)) {
            s->inst.d_lin_nl = s->ifam_nl();
            s->inst.d_lin_cones = s->inst.cones;
            s->inst.d_lin_knots = lin_d_knots(s);
            s->inst.d_lin_traj = lin_d_traj(s);
            s->inst.d_lin = solve_jit_supported(s->W, s->nx, s->nu, s->N, true, true, false, true, false, s->ifam_nl(), s->inst.cones, lin_d_knots(s), s->inst.d_lin_traj) ? 1 : 0;
        }
        return TINYMPC_OK;
    }
    decide_layout_d_variants(s);
    if ((rc = decide_layout_e(s))) return rc;
    return decide_layout_f(s);
}

// Slot refill (tinympc_solve_d.hip, REFILL): layout D's 16-lane kernels (box path), when the batch is more than the device holds at
// once and the tolerances can be met -- i.e. when instances finish at different times and there is something to refill a row
// with. TINYMPC_REFILL=0 switches it off, =1 takes it for any batch beyond one resident set whatever the tolerances. Shared tables, or
// the per-instance goal form (on by default as well: 65,536 quadrotors with a goal and a box each, 10.91 against 13.45 ms,
// profiles/refill_goal_ab.txt).
// The trajectory and per-knot bounds forms of the goal form (per-instance trajectories, tracks, bound schedules after tinympc_prepare)
// have a variant too, on by default as well: 65,536 quadrotors N=50 with a trajectory each, 7.45 against 19.71 ms, below the plain form
// in every round (profiles/refill_traj_ab.txt). Their resident set is their OWN plan's -- 4,096 instances where the form runs one
// wavefront per SIMD.
static bool refill_applies(const tinympc_solver *s, const LaunchPlan &pl) {
    const bool jit = pl.kernel == KernelId::D_JIT;
    if ((pl.kernel != KernelId::D_COMPILED && !jit) || s->W != 16 || pl.adaptive || pl.families || s->zero_copy_tick || s->st.max_iter <= 0 ||
        s->st.check_termination <= 0)
        return false;
    if (pl.inst_models) return false;  // (the model form has no slot-refill variant)
    // A per-instance handle: when the launch runs layout D's goal form (a row that takes an instance takes its four lane constants with
    // it), or that form on per-instance trajectories / tracks and / or bounds per knot (the row also restages its column of its
    // wavefront's linref / clamp rows); the per-instance families' form -- linear rows, with or without trajectories -- has no variant.
    const bool goal = pl.inst_refs;
    if (goal && pl.inst_lin) return false;
    const bool traj = goal && pl.inst_traj, kbnd = goal && pl.inst_kbnd;
    if ((traj || kbnd) && !jit) return false;  // (those forms are specialisations)
    const char *env = getenv("TINYMPC_REFILL");
    const int mode = env ? atoi(env) : -1;
    if (mode == 0) return false;
    const bool ct = s->tables_const() || goal;  // (the plan's constness: the goal form always has constant tables)
    long resident;  // wavefronts = groups of four instances
    if (jit) resident = solve_jit_resident_wavefronts(s->W, s->nx, s->nu, s->N, ct, goal, traj, kbnd);  // (the form's own plan: one wavefront per SIMD for the long trajectory forms)
    else {
        const int wpg = solve_d_wavefronts_per_workgroup(s->nu, s->N, ct);
        resident = (long)solve_d_resident_workgroups(wpg) * wpg;
    }
    // Tolerances nothing can meet (forced iteration counts): every instance runs max_iter, there is nothing to balance, and the
    // plain kernel's sweeps are the faster ones (65,536 x 200 iterations: 13.3 against 13.7 ms) -- keep it.
    const bool reachable = s->st.abs_pri_tol > 0.0 && s->st.abs_dua_tol > 0.0;
    if ((long)s->groups <= resident) return false;
    if (!reachable && mode != 1) return false;
    return !jit || solve_jit_refill_supported(s->W, s->nx, s->nu, s->N, ct, goal, traj, kbnd);  // (run-time specialised shapes: built on first use)
}

// Lean sweeps (tinympc_lean_d.hip, TINY_LEAN): layout D's compiled-in 16-lane kernels (box path; shared tables or the per-instance
// goal form), whenever some iteration's residuals cannot be read -- a check interval other than 1 (0: no check at all), or
// tolerances nothing can meet (forced iteration counts: only the last check of a launch reaches the statistics). With a check in
// every iteration and reachable tolerances every sweep needs its residuals and the plain kernel stays. Results are bit-identical.
// TINYMPC_LEAN=0 forces the plain kernel, =1 the lean one wherever it exists.
static bool lean_applies(const tinympc_solver *s, const LaunchPlan &pl) {
    if (pl.kernel != KernelId::D_COMPILED || s->W != 16 || pl.adaptive || pl.families || s->zero_copy_tick || s->st.max_iter <= 0)
        return false;
    if (pl.inst_models) return false;  // (the model form has no lean variant: it is a specialisation, never D_COMPILED)
    if (refill_applies(s, pl)) return false;
    const char *env = getenv("TINYMPC_LEAN");
    const int mode = env ? atoi(env) : -1;
    if (mode == 0) return false;
    if (mode == 1) return true;
    const bool reachable = s->st.abs_pri_tol > 0.0 && s->st.abs_dua_tol > 0.0;
    return s->st.check_termination != 1 || !reachable;
}
// ... and where they apply, the lean kernels are those of tinympc_lstart_d.hip (accumulator starts read from LDS, loop control out of
// the lean inner loop; bit-identical again). TINYMPC_LEAN_START=0 selects the lean kernels of tinympc_lean_d.hip.
static bool lean_start_applies() {
    const char *env = getenv("TINYMPC_LEAN_START");
    return !env || atoi(env) != 0;
}
// ... in their trimmed form (tinympc_ltrim_d.hip: the d stores of a lean round go through a per-lane address instead of a narrowed EXEC;
// bit-identical again). TINYMPC_LEAN_TRIM=0 selects the kernels of tinympc_lstart_d.hip.
static bool lean_trim_applies() {
    const char *env = getenv("TINYMPC_LEAN_TRIM");
    return lean_start_applies() && (!env || atoi(env) != 0);
}
// ... with d and the slack sharing the register slots inside a run of lean rounds (tinympc_lshare_d.hip; bit-identical again).
// TINYMPC_LEAN_SHARE=0 selects the kernels of tinympc_ltrim_d.hip.
static bool lean_share_applies() {
    const char *env = getenv("TINYMPC_LEAN_SHARE");
    return lean_trim_applies() && (!env || atoi(env) != 0);
}
// ... and, for the one shape that has LDS slots (quadrotor N=50, constant tables), with twelve of them turned into register slots
// inside a run of lean rounds (tinympc_lpark_d.hip; bit-identical again) -- where the run is long enough to pay for its entry and exit.
// A run of n rounds is n - 1 shared rounds, each 48 LDS instructions shorter than the shared kernels' (72 to 110 SIMD-cycles at the 1.5
// to 2.3 cycles per LDS instruction of docs/NOTEBOOK.md sections 14 and 18), and one last round; entry and exit cost 12 more reads of
// d, three stores and three reads of the parked values and one more wait for them, about 100 to 150 cycles: even at n = 3. The
// threshold is twice that and one more, PARK_MIN_RUN = 6 (at least 360 cycles saved against at most 150 spent); shorter runs keep the
// shared kernels. The length is that of the launch's first run, as the kernel's loop forms it: check_termination - 1 with tolerances
// that can be met, else up to the last check of the launch (max_iter - 1 where max_iter is a multiple of the interval).
// TINYMPC_LEAN_PARK=0 selects the kernels of tinympc_lshare_d.hip.
constexpr int PARK_MIN_RUN = 6;
static int first_lean_run(const tinympc_solver *s) {
    const int max_iter = s->st.max_iter, ct = s->st.check_termination;
    const bool reachable = s->st.abs_pri_tol > 0.0 && s->st.abs_dua_tol > 0.0;
    if (ct > 0 && reachable) return ct - 1 < max_iter ? ct - 1 : max_iter;
    const int last_check = ct > 0 ? (max_iter / ct) * ct : 0;
    return last_check > 0 ? last_check - 1 : max_iter;
}
static bool lean_park_applies(const tinympc_solver *s) {
    const char *env = getenv("TINYMPC_LEAN_PARK");
    if (!lean_share_applies() || (env && atoi(env) == 0)) return false;
    if (!(s->nx == 12 && s->nu == 4 && s->N == 50)) return false;
    return first_lean_run(s) >= PARK_MIN_RUN;
}
static const char *lean_words(const tinympc_solver *s, const LaunchPlan &pl) {
    const bool ct = s->tables_const() || (pl.inst_refs && pl.kernel != KernelId::A);  // (SolveParams::const_tables)
    return !lean_applies(s, pl)   ? ""
           : ct && lean_park_applies(s) ? " lean lds-start trim share park"
           : lean_share_applies() ? " lean lds-start trim share"
           : lean_trim_applies()  ? " lean lds-start trim"
           : lean_start_applies() ? " lean lds-start"
                                  : " lean";
}

// Everything launch() refuses, for plan `pl` of the current configuration: host-side tests only. launch() runs it before it queues or
// rebuilds anything; tinympc_rollout_batch runs it before tick 0, so that a refused rollout has queued nothing.
int check_launch(const tinympc_solver *s, const LaunchPlan &pl) {
    const bool fam = pl.families, adaptive = pl.adaptive;
    if (s->inst.fam() && !pl.inst_lin) {  // never a solve with shared rows or slopes in their place
        const char *why = s->layout_m ? "for systems with nx+nu > 64"
                          : s->inst.models ? (s->inst.rho_verb ? "with per-instance models or rho (set_model_batch / set_rho_batch); tinympc_clear_model_batch returns to the shared model and rho"
                                                               : "with per-instance models (set_model_batch); tinympc_clear_model_batch returns to the shared model")
                          : adaptive ? "with adaptive rho"
                                     : "with more cones or rounds of overlapping cones than the generic kernel holds";
        if (!s->inst.lin)
            return fail(TINYMPC_ERR_UNSUPPORTED, "per-instance cone slopes (set_cone_slopes_batch) are not supported %s; "
                        "tinympc_set_cone_constraints returns to shared slopes", why);
        return fail(TINYMPC_ERR_UNSUPPORTED, "per-instance linear constraints (%s)%s are not supported %s; "
                    "tinympc_set_linear_constraints returns to shared rows%s", s->inst.lin_knots ? "set_linear_constraints_knots_batch" : "set_linear_constraints_batch",
                    s->inst.cones ? " and cone slopes (set_cone_slopes_batch)" : "", why,
                    s->inst.cones ? ", tinympc_set_cone_constraints to shared slopes" : "");
    }
    if (s->inst_tables() && !pl.inst_refs) {  // never a solve with the shared references / bounds / model in their place
        const bool r = s->inst.refs(), b = s->inst.bounds, m = s->inst.models;
        const char *what[3], *back[3];
        int n = 0;
        if (r) { what[n] = "per-instance references (set_x_ref_batch / set_u_ref_batch)"; back[n++] = "tinympc_set_x_ref / tinympc_set_u_ref return to shared references"; }
        if (b) { what[n] = "per-instance bounds (set_bound_constraints_batch)"; back[n++] = "tinympc_set_bound_constraints returns to shared bounds"; }
        if (m) {  // (entered through tinympc_set_rho_batch: the message names that verb too)
            what[n] = s->inst.rho_verb ? "per-instance models (set_model_batch) with per-instance rho (set_rho_batch)" : "per-instance models (set_model_batch)";
            back[n++] = s->inst.rho_verb ? "tinympc_clear_model_batch returns to the shared model and rho" : "tinympc_clear_model_batch returns to the shared model";
        }
        std::string subj, way;
        for (int i = 0; i < n; ++i) {
            subj += std::string(i == 0 ? "" : i == n - 1 ? " and " : ", ") + what[i];
            way += std::string(i == 0 ? "" : ", ") + back[i];
        }
        return fail(TINYMPC_ERR_UNSUPPORTED, "%s are not supported %s; %s", subj.c_str(),
                    s->layout_m ? "for systems with nx+nu > 64" : fam ? "with cone / linear constraint families" : "with adaptive rho", way.c_str());
    }
    if (adaptive && fam)
        return fail(TINYMPC_ERR_UNSUPPORTED, "adaptive_rho together with cone / linear constraint families is not supported");
    if (s->layout_m && adaptive)
        return fail(TINYMPC_ERR_UNSUPPORTED, "adaptive_rho is not supported for systems with nx+nu > 64");
    if (fam && pl.kernel != KernelId::E && pl.kernel != KernelId::F && pl.kernel != KernelId::M && family_structure(s).beyond_generic())
        return fail(TINYMPC_ERR_UNSUPPORTED, "more than %d linear rows per side, %d cones or %d rounds of overlapping cones run on the run-time "
                    "specialised kernels only (nx+nu <= 16, TINYMPC_JIT not 0): this configuration has none (%s)", MAX_LIN_ROWS, MAX_CONES, MAX_ROUNDS,
                    s->W != 16 ? "nx+nu > 16" : "the specialiser refused it, see tinympc_get_jit_info");
    return TINYMPC_OK;
}

int launch(tinympc_solver *s, bool timed) {
    int rc;
    s->flag_pending = false;
    if ((rc = resolve_plan(s))) return rc;
    const LaunchPlan pl = current_plan(s);
    const bool fam = pl.families, adaptive = pl.adaptive;
    if ((rc = check_launch(s, pl))) return rc;
    // k_build_adapt reads the device copy of the references before the solve kernel starts: bring the device copies and the tables up
    // to date the ordinary way (every other kernel of a single-instance handle stages references left in pinned host memory itself)
    if (s->refs_on_host && (adaptive || pl.inst_models)) {  // (... and so are the per-instance rows of the models' variant)
        if ((rc = flush_host_refs(s))) return rc;
    }
    if ((rc = refresh_derived(s))) return rc;
    if (adaptive) {  // tiny tables from the current cache, sensitivities and Xref; rebuilt per launch (a few microseconds)
        AdaptTableParams a{};
        a.nx = s->nx; a.nu = s->nu; a.N = s->N; a.W = s->W; a.KT = s->KT;
        a.A = s->dA; a.B = s->dB; a.Pinf = s->dPinf; a.dK = s->ddK; a.dP = s->ddP; a.Xref = s->dXref; a.out = s->dadapt;
        HIP_TRY(launch_build_adapt(a, s->stream));
    }
    if (pl.inst_lin && (rc = refresh_inst_families(s))) return rc;  // (the store's copy of the shared rows, its slope vectors)
    if ((fam || pl.inst_lin) && (rc = refresh_families(s))) return rc;  // (per-instance linear rows: the kernel reads cones and enable flags there)
    if (pl.inst_refs && (rc = refresh_inst_tables(s))) return rc;
    SolveParams p{};
    p.nx = s->nx; p.nu = s->nu; p.N = s->N; p.batch = s->batch;
    p.max_iter = s->st.max_iter; p.check_termination = s->st.check_termination;
    p.rho = s->rho; p.abs_pri_tol = s->st.abs_pri_tol; p.abs_dua_tol = s->st.abs_dua_tol;
    p.ops = pl.inst_models ? s->inst.ops : s->dops;  // (per-instance models: every instance's own operator block)
    p.tables = s->dtables; p.x0 = s->dx0;
    p.groups = s->groups;
    p.G = s->dG; p.V = s->dV; p.V2 = s->dV2; p.D = s->dD; p.sol_x = s->dsolx; p.sol_u = s->dsolu;
    p.istats = s->distats; p.dstats = s->ddstats;
    p.tables_in_lds = pl.tables_in_lds ? 1 : 0;
    p.fam = s->dfam; p.GC = s->dGC; p.GL = s->dGL; p.LX = s->dLX;
    p.families = (fam || pl.inst_lin) ? 1 : 0;
    p.adaptive = adaptive ? 1 : 0;
    p.scratch = s->state_in_global ? s->dscratch_state : nullptr;
    if (s->layout_m && fam) {  // layout M with families: the forward sweep leaves its rollout x | u here for the families' phase
        if (!s->dscratch_state && (rc = dalloc(s, &s->dscratch_state, s->v_doubles()))) return rc;
        p.scratch = s->dscratch_state;
    }
#ifdef TINY_CLOCK_STAMP  // diagnostic build (tools/clock_check.py): layout D stamps its iteration loop into this buffer
    if (!s->state_in_global) {
        if (!s->dclock && (rc = dalloc(s, &s->dclock, (size_t)8 * s->groups))) return rc;
        p.scratch = s->dclock;
    }
#endif
    p.scratch_stride = state_scratch_doubles(s->nu, s->N, s->W);
    p.const_tables = (s->tables_const() || (pl.inst_refs && pl.kernel != KernelId::A)) ? 1 : 0;
    if (s->zero_copy_tick && pl.host_exchange) {  // set by tinympc_mpc_step_batch for the duration of one launch
        p.x0 = s->h_x0;
        p.x0_mirror = s->dx0;
        p.u0_host = s->h_u0;
    }
    if (s->host_path()) {
        if (s->x0_on_host) {
            p.x0 = s->h_x0;
            p.x0_mirror = s->dx0;
            s->x0_on_host = false;  // the kernel mirrors it into dx0
        }
        if (s->st.max_iter > 0) {   // (a 0-iteration solve writes nothing anywhere)
            p.host_sol = s->h_sol;
            s->host_sol_state = 1;
        }
    }
    if (s->refs_on_host) {  // (host_path() handles only: batch == 1, one workgroup)
        p.href_x = s->h_xref; p.href_u = s->h_uref;
        p.dXref = s->dXref; p.dUref = s->dUref; p.Pinf = s->dPinf;
        s->refs_on_host = false;  // the kernel brings the tables and the device copies up to date
    }
    p.adapt = s->dadapt; p.rho_inst = s->drho_inst;
    if (pl.inst_lin) { p.ilin = s->inst.lrows; p.ilin_nl = s->ifam_nl(); }  // (share the slots of adapt / chunk_len, which this kernel never reads)
    if (pl.inst_lin && s->inst.lin_knots) p.ilin_knots = s->inst.lin_knots;  // (rows per knot: the store's slots per group, in chunk_count's slot)
    if (pl.inst_models) p.rho_inst = s->inst.mrho;  // (the model kernels read rho per instance: the handle's, or what tinympc_set_rho_batch set)
    if (pl.inst_refs) {
        // (layout A and layout D's trajectory form: the rows of every knot; the goal form: knot 0's)
        p.iref_lr = (pl.kernel == KernelId::A || pl.inst_traj) ? s->inst.lr_rows() : s->inst.lrg;
        p.iref_pn = s->inst.pn;
        if (pl.inst_kbnd) p.ibnd = s->inst.bnd;  // (layout D's per-knot bounds form: layout A's clamp rows, every knot's)
        else if (pl.kernel != KernelId::A) p.ibnd = s->inst.bndg;  // (the goal form: always per lane)
        else if (pl.inst_bounds) p.ibnd = s->inst.bnd;
    }
    p.rho_min = s->st.adaptive_rho_min; p.rho_max = s->st.adaptive_rho_max; p.rho_clip = s->st.adaptive_rho_enable_clipping;
    // a pending cold start: layout D's kernels start from zero registers; every other kernel loads its state from HBM
    // (a solve of zero iterations writes nothing back: the zeros must then be in HBM)
    const bool kernel_takes_cold = (pl.kernel == KernelId::D_COMPILED || pl.kernel == KernelId::D_JIT) && s->st.max_iter > 0;
    if (s->cold_state && !kernel_takes_cold && (rc = materialize_cold_state(s))) return rc;
    p.cold = s->cold_state ? 1 : 0;
    s->cold_state = false;  // (the launch below writes the state back)
    if (s->st.max_iter > 0) s->sol_zero_pending = false;  // (every instance writes its whole solution)
    else if ((rc = materialize_zero_solution(s))) return rc;
    if (refill_applies(s, pl) && !p.x0_mirror && !p.u0_host && !p.host_sol) {  // slot refill (see refill_applies)
        if (!s->drefill && (rc = dalloc(s, &s->drefill, 1))) return rc;
        HIP_TRY(hipMemsetAsync(s->drefill, 0, sizeof(int), s->stream));
        p.refill_next = s->drefill;
    }
    if (timed) HIP_TRY(hipEventRecord(s->ev0, s->stream));
    switch (pl.kernel) {
        case KernelId::M:
            p.ctab = s->dctab;  // (beyond 128 rows: the tile-major copy of the operators; NULL otherwise)
            HIP_TRY(launch_solve_m(p, s->stream));
            break;
        case KernelId::D_JIT:  // (box path, families with everything in registers, or adaptive rho per lane)
            HIP_TRY(launch_solve_jit(p, s->W, s->stream, pl.inst_models, pl.inst_lin ? s->ifam_nl() : 0, pl.inst_lin && s->inst.cones, pl.inst_lin ? lin_d_knots(s) : 0,
                                     pl.inst_traj, pl.inst_kbnd));
            break;
        case KernelId::D_COMPILED:
            if (lean_applies(s, pl) && !p.x0_mirror && !p.u0_host && !p.refill_next)
                HIP_TRY(p.const_tables && lean_park_applies(s) ? launch_solve_d_lean_park(p, s->stream)
                        : lean_share_applies() ? launch_solve_d_lean_share(p, s->stream)
                        : lean_trim_applies()  ? launch_solve_d_lean_trim(p, s->stream)
                        : lean_start_applies() ? launch_solve_d_lean_start(p, s->stream)
                                               : launch_solve_d_lean(p, s->stream));
            else HIP_TRY(s->W == 64 ? launch_solve_dx(p, s->stream) : s->W == 32 ? launch_solve_dw(p, s->stream) : launch_solve_d(p, s->stream));
            break;
        case KernelId::E:
            p.ctab = s->dctab_e; p.chunk_len = s->e_chunk_len; p.chunk_count = s->e_wpg; p.chunk_levels = 1;
            HIP_TRY(launch_solve_e(p, s->fs, s->stream));
            break;
        case KernelId::F:
            p.ctab = s->dctab_f; p.ftab = s->dftab; p.chunk_len = s->f_chunk_len; p.chunk_count = s->f_chunks; p.chunk_levels = 4;
            arm_completion_flag(s, p);
            HIP_TRY(launch_solve_f(p, s->f_fs, s->stream));
            break;
        case KernelId::C:  // (with the families: the latency kernel carries them itself, same HBM state as k_admm_solve_fam)
            p.ctab = s->dctab; p.chunk_len = s->chunk_len; p.chunk_count = s->chunk_count; p.chunk_levels = s->chunk_levels;
            arm_completion_flag(s, p);
            HIP_TRY(launch_solve_c(p, s->W, s->KT, s->lds_bytes_c, s->stream));
            break;
        case KernelId::B:
            HIP_TRY(launch_solve_b(p, s->W, s->KT, s->lds_bytes, s->stream));
            break;
        case KernelId::A:
        case KernelId::FAM_A:  // (the families and adaptive rho share the persistent state -- G, canonical V, D -- with every other kernel)
        case KernelId::ADAPT_A: {
            const SolveExt ext = pl.kernel == KernelId::FAM_A ? SolveExt::Families : pl.kernel == KernelId::ADAPT_A ? SolveExt::Adaptive
                                 : pl.inst_lin ? (s->inst.lin_knots ? SolveExt::InstFamiliesKnots : SolveExt::InstFamilies) : pl.inst_models ? SolveExt::InstModels : pl.inst_bounds ? SolveExt::InstBounds : pl.inst_refs ? SolveExt::InstRefs : SolveExt::Box;
            HIP_TRY(launch_solve_a(p, ext, s->W, s->KT, s->lds_bytes_a, s->stream));
            break;
        }
    }
    if (timed) HIP_TRY(hipEventRecord(s->ev1, s->stream));
    return TINYMPC_OK;
}

}  // namespace host
}  // namespace tinympc

extern "C" {

int tinympc_get_launch_info(tinympc_solver *s, int *lanes_per_instance, int *instances_per_wave, int *workgroups,
                            int *lds_bytes, int *tables_in_lds) {
    int rc = check_handle(s);
    if (rc) return rc;
    const LaunchPlan pl = current_plan(s);
    if (lanes_per_instance) *lanes_per_instance = s->W;
    if (instances_per_wave) *instances_per_wave = s->IPW;
    if (workgroups) *workgroups = pl.workgroups;
    if (lds_bytes) *lds_bytes = (int)pl.lds_bytes;
    if (tables_in_lds) *tables_in_lds = pl.tables_in_lds ? 1 : 0;  // (layouts C - F keep their table entries in registers or copy them themselves)
    return TINYMPC_OK;
}

int tinympc_get_layout(tinympc_solver *s) {
    if (!s) return 0;
    return current_plan(s).layout;
}

int tinympc_prepare(tinympc_solver *s) {
    int rc = check_handle(s);
    if (rc) return rc;
    if ((rc = bind_device(s))) return rc;
    s->specialise_asked = true;  // (the caller pays for specialised kernels now: layout F for the box path of small batches)
    if ((rc = resolve_plan(s))) return rc;
    (void)refill_applies(s, current_plan(s));  // (a run-time specialised shape builds its slot-refill variant here, not in the first solve)
    return TINYMPC_OK;
}

static int jit_info_text(tinympc_solver *s, char *buf, int len);

int tinympc_get_jit_info(tinympc_solver *s, char *buf, int len) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (!buf || len < 1) return fail(TINYMPC_ERR_INVALID_INPUT, "get_jit_info: buffer required");
    buf[0] = '\0';
    if ((rc = jit_info_text(s, buf, len))) return rc;
    if (s->inst.tracks()) strncat(buf, " reference-track", (size_t)len - strlen(buf) - 1);  // (a half is in track mode)
    if (s->inst.lin) strncat(buf, s->inst.lin_knots ? " per-knot-linear" : " per-instance-linear", (size_t)len - strlen(buf) - 1);
    if (s->inst.cones) strncat(buf, " per-instance-cones", (size_t)len - strlen(buf) - 1);
    // (the families' form on per-instance trajectories / tracks, taken or asked for and refused: behind the mode's own words)
    if (s->inst.fam() && lin_wants_d(s) && lin_d_traj(s) && s->inst.d_lin >= 0 && lin_d_answer_current(s))
        strncat(buf, " per-instance-trajectories", (size_t)len - strlen(buf) - 1);
    return TINYMPC_OK;
}

static int jit_info_text(tinympc_solver *s, char *buf, int len) {
    int rc;
    const LaunchPlan pl = current_plan(s);
    const bool ct = s->tables_const();
    if (pl.inst_refs) {
        // (per-instance-refs only when references are per instance; per-instance-bounds only when bounds are)
        const std::string w = std::string(s->inst.refs() ? " per-instance-refs" : "") + (s->inst.bounds ? " per-instance-bounds" : "") +
                              (pl.inst_models ? " per-instance-models" : "");
        const char *words = w.c_str();
        if (!pl.inst_lin && !pl.inst_models && (pl.inst_kbnd || (pl.kernel == KernelId::A && kbnd_wants_d(s) && s->inst.d_kbnd == 0 && s->inst.d_kbnd_traj == kbnd_traj(s)))) {
            // layout D's per-knot bounds form -- or asked for and refused (a plan, but no kernel): layout A, and why
            if ((rc = bind_device(s))) return rc;
            const bool tr = kbnd_traj(s);
            solve_jit_describe(s->W, s->nx, s->nu, s->N, true, false, false, buf, (size_t)len, true, false, 0, false, 0, tr, true);
            strncat(buf, words, (size_t)len - strlen(buf) - 1);
            if (tr) strncat(buf, " per-instance-trajectories", (size_t)len - strlen(buf) - 1);
            strncat(buf, " per-knot-bounds", (size_t)len - strlen(buf) - 1);
            if (pl.kernel == KernelId::D_JIT && refill_applies(s, pl)) strncat(buf, " slot-refill", (size_t)len - strlen(buf) - 1);
        } else if (pl.kernel == KernelId::D_JIT && pl.inst_traj && !pl.inst_lin) {  // layout D's trajectory form (box path)
            if ((rc = bind_device(s))) return rc;
            solve_jit_describe(s->W, s->nx, s->nu, s->N, true, false, false, buf, (size_t)len, true, false, 0, false, 0, true);
            strncat(buf, words, (size_t)len - strlen(buf) - 1);
            strncat(buf, " per-instance-trajectories", (size_t)len - strlen(buf) - 1);
            if (refill_applies(s, pl)) strncat(buf, " slot-refill", (size_t)len - strlen(buf) - 1);
        } else if (pl.kernel == KernelId::A && !pl.inst_lin && !pl.inst_models && traj_wants_d(s) && s->inst.d_traj == 0) {  // asked for and refused: layout A, and why
            if ((rc = bind_device(s))) return rc;
            solve_jit_describe(s->W, s->nx, s->nu, s->N, true, false, false, buf, (size_t)len, true, false, 0, false, 0, true);
            strncat(buf, words, (size_t)len - strlen(buf) - 1);
            strncat(buf, " per-instance-trajectories", (size_t)len - strlen(buf) - 1);
        } else if (pl.kernel == KernelId::D_JIT) {
            if ((rc = bind_device(s))) return rc;
            const int ilin = pl.inst_lin ? s->ifam_nl() : 0;
            solve_jit_describe(s->W, s->nx, s->nu, s->N, true, ilin != 0, false, buf, (size_t)len, true, pl.inst_models, ilin, ilin && s->inst.cones, ilin ? lin_d_knots(s) : 0,
                               pl.inst_traj);
            strncat(buf, words, (size_t)len - strlen(buf) - 1);
            if (!pl.inst_traj) strncat(buf, " goal", (size_t)len - strlen(buf) - 1);  // (the families' form on trajectories, inst_lin with inst_traj: named behind the mode's words)
            if (refill_applies(s, pl)) strncat(buf, " slot-refill", (size_t)len - strlen(buf) - 1);  // (the goal form of the box path, not the families': see refill_applies)
        } else if (pl.inst_lin && lin_wants_d(s) && s->inst.d_lin == 0 && lin_d_answer_current(s)) {  // asked for and refused: layout A, and why
            if ((rc = bind_device(s))) return rc;
            solve_jit_describe(s->W, s->nx, s->nu, s->N, true, true, false, buf, (size_t)len, true, false, s->ifam_nl(), s->inst.cones, lin_d_knots(s), lin_d_traj(s));
            strncat(buf, words, (size_t)len - strlen(buf) - 1);
        } else if (pl.inst_lin && lin_runs(s) && s->specialise_asked && s->layout_d && s->W == 16 && lin_refs_fit_d(s) && family_structure(s).nround > 1) {
            // asked for, and only the cones keep the mode off layout D: layout A, and why
            snprintf(buf, (size_t)len, "refused(cones that share rows run in rounds: layout D's per-instance form takes cones without rounds) layout=%c%s",
                     pl.layout, words);
        } else if (pl.inst_models && models_want_d(s) && s->inst.d_models == 0) {  // asked for and refused: layout A, and why
            if ((rc = bind_device(s))) return rc;
            solve_jit_describe(s->W, s->nx, s->nu, s->N, true, false, false, buf, (size_t)len, false, true);
            strncat(buf, words, (size_t)len - strlen(buf) - 1);
        } else {
            snprintf(buf, (size_t)len, "compiled-in layout=%c%s%s%s%s", pl.layout, words, pl.kernel == KernelId::D_COMPILED ? " goal" : "",
                     refill_applies(s, pl) ? " slot-refill" : "", lean_words(s, pl));
            // (the per-knot bounds form was asked for and the horizon's clamp rows fit no plan: layout A, nothing was refused)
            if (pl.kernel == KernelId::A && kbnd_wants_d(s) && s->inst.d_kbnd == 2 && s->inst.d_kbnd_traj == kbnd_traj(s))
                strncat(buf, " per-knot-bounds(no plan)", (size_t)len - strlen(buf) - 1);
        }
        return TINYMPC_OK;
    }
    // a specialisation that was asked for and refused leaves the plan on a generic kernel: say why
    if (!pl.adaptive && !s->f_sig.empty() && !s->f_ok && pl.kernel != KernelId::E && pl.kernel != KernelId::D_JIT && pl.kernel != KernelId::D_COMPILED)
        solve_f_describe(s->nx, s->nu, s->N, ct, pl.families, s->f_fs, buf, (size_t)len);
    else if (!pl.adaptive && !s->e_sig.empty() && !s->e_ok && pl.kernel != KernelId::F && pl.kernel != KernelId::D_JIT && pl.kernel != KernelId::D_COMPILED)
        solve_e_describe(s->nx, s->nu, s->N, ct, pl.families, s->fs, buf, (size_t)len);
    else if (pl.kernel == KernelId::F) solve_f_describe(s->nx, s->nu, s->N, ct, pl.families, s->f_fs, buf, (size_t)len);
    else if (pl.kernel == KernelId::E) solve_e_describe(s->nx, s->nu, s->N, ct, pl.families, s->fs, buf, (size_t)len);
    else if (pl.kernel == KernelId::D_JIT || (s->d_jit_asked && !s->layout_d && !s->layout_m)) {
        if ((rc = bind_device(s))) return rc;
        solve_jit_describe(s->W, s->nx, s->nu, s->N, ct, pl.families && !pl.adaptive, pl.adaptive && !pl.families, buf, (size_t)len);
        if (pl.kernel == KernelId::D_JIT && refill_applies(s, pl)) strncat(buf, " slot-refill", (size_t)len - strlen(buf) - 1);
    } else snprintf(buf, (size_t)len, "compiled-in layout=%c%s%s", pl.layout, refill_applies(s, pl) ? " slot-refill" : "",
                  lean_words(s, pl));
    return TINYMPC_OK;
}

}  // extern "C"
