// tinympc_capi.hip -- the verbs of the extern "C" boundary declared in include/tinympc_hip.h: argument validation with the
// reference's error behaviour, data in and out. The handle and its helpers: tinympc_handle.h / .hip; which kernel a launch runs:
// tinympc_plan.hip; the resident session: tinympc_session.hip. Host-side bookkeeping only -- every number the solver produces is
// computed by the kernels; there is no CPU fallback anywhere.
#include "tinympc_handle.h"
#include "tinympc_rollout.h"

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <new>

using namespace tinympc;
using namespace tinympc::host;

extern "C" {

const char *tinympc_last_error(void) { return last_error_slot().c_str(); }
int tinympc_abi_version(void) { return TINYMPC_ABI_VERSION; }

int tinympc_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int tinympc_setup_batch(tinympc_solver **out, const double *A, const double *B, const double *fdyn,
                        const double *Q, const double *R, double rho, int nx, int nu, int N, int batch,
                        int device, int verbose) {
    if (!out) return fail(TINYMPC_ERR_INVALID_INPUT, "setup: output handle pointer is NULL");
    *out = nullptr;
    if (!A || !B || !Q || !R) return fail(TINYMPC_ERR_INVALID_INPUT, "setup requires A, B, Q, R");
    if (nx < 1 || nu < 1) return fail(TINYMPC_ERR_INVALID_INPUT, "setup: nx and nu must be >= 1 (got %d, %d)", nx, nu);
    if (N < 2) return fail(TINYMPC_ERR_INVALID_INPUT, "setup: N must be >= 2 (TinyMPC.m:52), got %d", N);
    if (batch < 1) return fail(TINYMPC_ERR_INVALID_INPUT, "setup: batch must be >= 1, got %d", batch);
    int W = 0, KT = 0;
    const bool large = solve_m_supported(nx, nu);
    if (large) {
        W = KT = solve_m_geometry(nx, nu);  // geometry of the operators / tables (128, 256 or 512); the kernel works on 16-instance tiles
    } else if (!choose_geometry(nx, nu, &W, &KT)) {
        return fail(TINYMPC_ERR_UNSUPPORTED, "nx+nu = %d: systems beyond 512 rows are not supported by this build", nx + nu);
    }
    int ndev = tinympc_device_count();
    if (ndev < 1) return fail(TINYMPC_ERR_NO_DEVICE, "no HIP device visible: the HIP path has no CPU fallback");
    if (device >= ndev) return fail(TINYMPC_ERR_INVALID_INPUT, "device %d out of range (have %d)", device, ndev);

    tinympc_solver *s = new (std::nothrow) tinympc_solver();
    if (!s) return fail(TINYMPC_ERR_ALLOC, "out of host memory");
    const auto t_setup = std::chrono::steady_clock::now();
    if (device < 0) {
        if (hipGetDevice(&s->device) != hipSuccess) s->device = 0;
    } else {
        s->device = device;
    }
    s->nx = nx; s->nu = nu; s->N = N; s->batch = batch; s->rho = rho;
    s->W = W; s->KT = KT;
    s->layout_m = large;
    s->IPW = large ? 16 : 64 / W;
    s->groups = (batch + s->IPW - 1) / s->IPW;  // wave groups; tiles of 16 instances for the large-system kernel
    // tiny_set_default_settings (tiny_api.cpp:213-231, tiny_api_constants.hpp:5-10)
    s->st = Settings{1e-3, 1e-3, 1000, 1, 1, 1, 0, 0, 0, 0, 0, 1.0, 100.0, 1};

    int rc = TINYMPC_OK;
#define TRY(x)            \
    do {                  \
        rc = (x);         \
        if (rc) {         \
            destroy(s);   \
            return rc;    \
        }                 \
    } while (0)
#define HIP_TRY_S(expr)                                                                              \
    do {                                                                                             \
        hipError_t e__ = (expr);                                                                     \
        if (e__ != hipSuccess) {                                                                     \
            destroy(s);                                                                              \
            return fail(TINYMPC_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e__));            \
        }                                                                                            \
    } while (0)

    HIP_TRY_S(hipSetDevice(s->device));
    park_sessions_on_device(s->device, s);  // (the allocations below synchronise the device)
    TRY(acquire_stream_kit(s));

    // LDS plan: ADMM state always; the per-knot tables too when the total fits the 160 KB of a CU.
    // (the large-system kernel plans its own LDS: everything below describes layouts A - D and stays unused for it)
    const int Wp = large ? 64 : W;
    const size_t with_tables = solve_lds_bytes(nx, nu, N, Wp, true);
    const size_t without = solve_lds_bytes(nx, nu, N, Wp, false);
    constexpr size_t kLdsMax = 160 * 1024;
    // Horizons whose state does not fit a CU's LDS run the same kernels on an HBM working copy (GMEM variant).
    s->state_in_global = !large && without > kLdsMax;
    if (const char *e = getenv("TINYMPC_STATE_GLOBAL")) s->state_in_global = !large && (e[0] == '1' || s->state_in_global);  // (experiments: the HBM working copy also where LDS would hold the state)
    // Two workgroups per CU need <= 80 KB each; prefer LDS tables whenever they do not cost a workgroup slot.
    const size_t slots_without = s->state_in_global ? 0 : kLdsMax / without;
    const size_t slots_with = kLdsMax / with_tables;
    // (up to four: one wavefront per SIMD. Wide systems -- 2 or 1 instances per wavefront -- have short state arrays and
    // long tables; keeping the tables in L2 doubles their wavefronts per CU, profiles/r02_wide_sweep.txt)
    s->tables_in_lds = !s->state_in_global && (with_tables <= kLdsMax) && (slots_with >= (slots_without > 4 ? 4 : slots_without));
    s->lds_bytes = s->state_in_global ? 0 : (s->tables_in_lds ? with_tables : without);
    s->lds_bytes_a = s->lds_bytes;
    s->tables_in_lds_a = s->tables_in_lds;
    // Layout A keeps all ADMM state in LDS (2 wavefronts per CU at quadrotor size); layout B keeps V as an
    // L2-resident ping-pong pair in HBM and fits 4 wavefronts per CU. Measured on MI355X (quadrotor N=50):
    // B is 1.72x faster on a GPU-filling batch (5.56 vs 9.57 ms per 8192 x 200 iterations) and also
    // 13 % faster for a single instance (fewer LDS instructions per step), so B is used whenever it fits.
    // TINYMPC_LAYOUT=A|B overrides the choice (kernel A/B experiments, and the tests cover both).
    {
        const size_t b_bytes = solve_b_lds_bytes(nx, nu, N, W);
        const bool b_possible = (W == 16) && (N >= 8) && (b_bytes <= kLdsMax);
        bool want_b = b_possible;
        if (const char *env = getenv("TINYMPC_LAYOUT")) {
            if (env[0] == 'A' || env[0] == 'a') want_b = false;
            if ((env[0] == 'B' || env[0] == 'b') && b_possible) want_b = true;
        }
        if (want_b) {
            s->layout_b = true;
            s->tables_in_lds = true;
            s->lds_bytes = b_bytes;
        }
        // Layout C gives every instance a whole workgroup and cuts the horizon into 16 concurrent chunks: a
        // 2-3x shorter iteration for one instance, lower throughput once the batch fills the chip's wave slots.
        // Default for small batches; TINYMPC_LAYOUT=C forces it, =A / =B exclude it.
        chunk_plan(N, &s->chunk_len, &s->chunk_count, &s->chunk_levels);
        // (single-instance handles stage their references in LDS, see k_admm_solve_c's prologue)
        s->lds_bytes_c = batch == 1 ? solve_c_lds_bytes_refs(nx, nu, N, s->chunk_levels) : solve_c_lds_bytes(nx, s->chunk_levels);
        const bool c_possible = (W == 16) && (s->chunk_len <= 8) && (s->lds_bytes_c <= kLdsMax);
        bool want_c = c_possible && batch <= kLayoutCBatchMax;
        if (const char *env = getenv("TINYMPC_LAYOUT")) {
            if (env[0] == 'C' || env[0] == 'c') want_c = c_possible;
            else if (env[0] == 'A' || env[0] == 'a' || env[0] == 'B' || env[0] == 'b' || env[0] == 'D' || env[0] == 'd') want_c = false;
        }
        s->layout_c = want_c;
        // Layout D (compile-time shape, duals in registers, two wavefronts per SIMD): default above the latency kernel's
        // range -- for wide systems, which have no latency kernel, from 16 instances up --; TINYMPC_LAYOUT=D forces it at any
        // batch size (tests), =A / =B / =C exclude it. The shapes compiled into the library run as they are; every other
        // shape that fits the plan is specialised at run time (tinympc_jit.hip: hiprtc, cached), now, so that a failure
        // simply leaves the handle on layout B / A.
        const bool d_compiled = (W == 16 && solve_d_supported(nx, nu, N, true)) || (W == 32 && solve_dw_supported(nx, nu, N, true)) ||
                                (W == 64 && solve_dx_supported(nx, nu, N, true));
        bool want_d = (W == 16) ? !want_c : (batch >= 16 && !large);
        if (const char *env = getenv("TINYMPC_LAYOUT")) want_d = (env[0] == 'D' || env[0] == 'd');
        if (want_d && !d_compiled) {
            HIP_TRY_S(hipSetDevice(s->device));
            s->d_jit_asked = true;
            s->d_jit = solve_jit_supported(W, nx, nu, N, true);
            want_d = s->d_jit;
        }
        s->layout_d = want_d;
        if (want_d) s->layout_c = false;
        // The families: k_admm_solve_fam keeps the whole ADMM state in LDS (layout A), so a long horizon leaves it
        // one wavefront = 4 instances per CU; the latency kernel then wins at EVERY batch size (rocket N=100:
        // 30 vs 15.6 M iterations/s at 4096 instances, profiles/r01d_rocket_sweep.txt). Otherwise as for the box path.
        bool c_excluded = false;
        if (const char *env = getenv("TINYMPC_LAYOUT")) c_excluded = (env[0] == 'A' || env[0] == 'a' || env[0] == 'B' || env[0] == 'b' || env[0] == 'D' || env[0] == 'd');
        const size_t fam_a_waves_per_cu = s->state_in_global ? 1 : kLdsMax / (s->lds_bytes_a ? s->lds_bytes_a : kLdsMax);
        s->fam_c = c_possible && !c_excluded && (want_c || fam_a_waves_per_cu <= 1);
        s->c_tables = s->layout_c || s->fam_c;
    }

    const size_t X = s->X(), U = s->U();
    using clk = std::chrono::steady_clock;
    auto us_since = [](clk::time_point t) { return std::chrono::duration<double, std::micro>(clk::now() - t).count(); };
    s->setup_us[0] = us_since(t_setup);  // device, stream, events, the layout decisions above
    auto t_phase = clk::now();
    // ---- ONE block of device memory (ArenaPlan, tinympc_handle.h). Three spans:
    //   upload: the problem data, in the order of the pinned staging copy (one H2D copy below)
    ArenaPlan up;
    double *uA = nullptr, *uB = nullptr, *uf = nullptr, *uQd = nullptr, *uRd = nullptr, *uQ = nullptr, *uR = nullptr;  // staging slots
    up.add(&uA, (size_t)nx * nx); up.add(&uB, (size_t)nx * nu); up.add(&uf, nx); up.add(&uQd, nx); up.add(&uRd, nu);
    up.add(&uQ, (size_t)nx * nx); up.add(&uR, (size_t)nu * nu);
    const size_t upload_bytes = up.mark();
    ArenaPlan dev;
    dev.add(&s->dA, (size_t)nx * nx); dev.add(&s->dB, (size_t)nx * nu); dev.add(&s->dfdyn, nx); dev.add(&s->dQd, nx); dev.add(&s->dRd, nu);
    dev.add(&s->dQfull, (size_t)nx * nx); dev.add(&s->dRfull, (size_t)nu * nu);
    if (dev.mark() != upload_bytes) { destroy(s); return fail(TINYMPC_ERR_ALLOC, "setup: arena plans disagree"); }
    //   zeroed: everything tiny_setup zeroes (tiny_api.cpp:41-44, 73-88, 100-111) -- one memset
    const size_t zero_begin = dev.mark();
    dev.add(&s->ddK, (size_t)nu * nx); dev.add(&s->ddP, (size_t)nx * nx);
    dev.add(&s->dXref, X); dev.add(&s->dUref, U); dev.add(&s->dx0, (size_t)batch * nx);
    dev.add(&s->dG, s->state_doubles()); dev.add(&s->dV, s->v_doubles()); dev.add(&s->dV2, s->v_doubles()); dev.add(&s->dD, s->d_doubles());
    dev.add(&s->dsolx, X * batch); dev.add(&s->dsolu, U * batch);
    dev.add(&s->distats, (size_t)batch * 2); dev.add(&s->ddstats, (size_t)batch * 4);
    dev.add(&s->drefill, 1);
    const size_t zero_end = dev.mark();
    //   the rest: written by a kernel before anything reads it
    dev.add(&s->dKinf, (size_t)nu * nx); dev.add(&s->dPinf, (size_t)nx * nx);
    dev.add(&s->dQuu, (size_t)nu * nu); dev.add(&s->dAmBKt, (size_t)nx * nx);
    dev.add(&s->dAPf, nx); dev.add(&s->dBPf, nu); dev.add(&s->dinfo, 4);
    dev.add(&s->dscratch, (large ? precompute_large_scratch_doubles(nx, nu) : precompute_scratch_doubles(nx, nu)) + 8);
    dev.add(&s->dadapt, adapt_doubles(W, KT)); dev.add(&s->drho_inst, batch);
    if (s->c_tables) dev.add(&s->dctab, chunk_table_doubles(nx, s->chunk_levels));
    if (large && solve_m_tiled_ops_doubles(nx, nu)) dev.add(&s->dctab, solve_m_tiled_ops_doubles(nx, nu));  // layout M beyond 128 rows: tile-major operators
    dev.add(&s->dlqr_scratch, lqr_scratch_doubles(nx, nu) + 8); dev.add(&s->dlqr_out, 3 * s->cache_doubles());
    dev.add(&s->dxmin, X); dev.add(&s->dxmax, X); dev.add(&s->dumin, U); dev.add(&s->dumax, U);
    dev.add(&s->dops, ops_doubles(W, KT)); dev.add(&s->dtables, tables_doubles(W, N));
    if (s->state_in_global) dev.add(&s->dscratch_state, (size_t)s->groups * state_scratch_doubles(nu, N, W));
    if (!large && W == 16) {  // layouts E / F: the chunk operators of their plans (tinympc_plan.hip builds them at the launch that needs them)
        dev.add(&s->dctab_e, chunk_table_doubles(nx, 1)); dev.add(&s->dctab_f, chunk_table_doubles(nx, 4));
    }
    // ---- ... and ONE block of pinned host memory: the staging copy of the problem data and, for a single-instance handle, everything
    // the host and a running kernel exchange (coherent: see kBoundInf's neighbour comment in tinympc_handle.h)
    ArenaPlan pin;
    pin.add(&s->h_stage, upload_bytes / sizeof(double));
    if (batch == 1) {
        pin.add(&s->h_sol, X + U + 8); pin.add(&s->h_x0, nx); pin.add(&s->h_u0, nu);
        pin.add(&s->h_xref, X); pin.add(&s->h_uref, U ? U : 1); pin.add(&s->h_mail, 64); pin.add(&s->h_ans, 32);
    }
    TRY(acquire_arenas(s, dev.mark(), pin.mark(), batch == 1));
    dev.bind(s->arena_dev);
    s->setup_us[1] = us_since(t_phase); t_phase = clk::now();
    pin.bind(s->arena_pin);
    std::memset(s->arena_pin, 0, pin.total);  // h_sol, the references (tiny_api.cpp:83-84) and the mailbox start as zeros
    s->setup_us[2] = us_since(t_phase); t_phase = clk::now();
    // Problem data. Only the diagonals of Q and R are kept, each + rho (tiny_api.cpp:90-91).
    up.bind(s->h_stage);
    std::memcpy(uA, A, sizeof(double) * nx * nx); std::memcpy(uB, B, sizeof(double) * nx * nu);
    if (fdyn) std::memcpy(uf, fdyn, sizeof(double) * nx);
    for (int i = 0; i < nx; ++i) uQd[i] = Q[i + (size_t)i * nx] + rho;
    for (int i = 0; i < nu; ++i) uRd[i] = R[i + (size_t)i * nu] + rho;
    std::memcpy(uQ, Q, sizeof(double) * nx * nx); std::memcpy(uR, R, sizeof(double) * nu * nu);
    if (zero_end - zero_begin <= ((size_t)1 << 20)) {
        // a small handle: ONE launch does the upload (reading the pinned staging copy itself), the zeroing, the fills (k_setup_init)
        SetupInitParams ip{};
        ip.stage = s->h_stage; ip.upload_dst = s->dA; ip.upload_doubles = upload_bytes / sizeof(double);
        ip.zero = reinterpret_cast<double *>(static_cast<char *>(s->arena_dev) + zero_begin); ip.zero_doubles = (zero_end - zero_begin) / sizeof(double);
        ip.xmin = s->dxmin; ip.xmax = s->dxmax; ip.umin = s->dumin; ip.umax = s->dumax; ip.X = X; ip.U = U; ip.inf = kBoundInf;  // TinyMPC.m:261-264
        ip.rho_inst = s->drho_inst; ip.batch = batch; ip.rho = rho; ip.mail = s->d_mail;
        HIP_TRY_S(launch_setup_init(ip, s->stream));
    } else {
        HIP_TRY_S(hipMemcpyAsync(s->dA, s->h_stage, upload_bytes, hipMemcpyHostToDevice, s->stream));
        HIP_TRY_S(hipMemsetAsync(static_cast<char *>(s->arena_dev) + zero_begin, 0, zero_end - zero_begin, s->stream));
        if (s->d_mail) HIP_TRY_S(hipMemsetAsync(s->d_mail, 0, sizeof(double) * 64, s->stream));
        HIP_TRY_S(launch_fill_bounds(s->dxmin, s->dxmax, X, s->dumin, s->dumax, U, kBoundInf, s->stream));  // TinyMPC.m:261-264
        HIP_TRY_S(launch_reset_stats(s->distats, s->ddstats, s->drho_inst, batch, rho, s->stream));
    }
    s->setup_us[3] = us_since(t_phase); t_phase = clk::now();
    TRY(run_precompute(s));  // tiny_api.cpp:113
    s->setup_us[4] = us_since(t_phase); t_phase = clk::now();
    HIP_TRY_S(hipStreamSynchronize(s->stream));
    s->setup_us[5] = us_since(t_phase);
    s->setup_us[6] = us_since(t_setup);
#undef TRY
#undef HIP_TRY_S
    if (verbose) {
        int steps = 0;
        download(s, &steps, s->dinfo, sizeof(int));
        printf("TinyMPC-HIP setup: nx=%d nu=%d N=%d rho=%g batch=%d device=%d | lanes/instance=%d LDS=%zu B tables_in_lds=%d | Kinf converged after %d iterations\n",
               nx, nu, N, rho, batch, s->device, s->W, s->lds_bytes, (int)s->tables_in_lds, steps);
    }
    *out = s;
    return TINYMPC_OK;
}

int tinympc_setup(tinympc_solver **out, const double *A, const double *B, const double *fdyn,
                  const double *Q, const double *R, double rho, int nx, int nu, int N, int verbose) {
    return tinympc_setup_batch(out, A, B, fdyn, Q, R, rho, nx, nu, N, 1, -1, verbose);
}

// While measurement noise is on (tinympc_set_rollout_noise) the handle keeps the TRUE state in rn_px and the measurement in x0. A verb that
// writes x0 from outside restarts the true state of the instances it names from what it wrote: the same range, copied on the stream behind
// the write (a range and not a flag for the whole batch: the other instances' true state is not their measurement).
static int mirror_x0_into_px(tinympc_solver *s, int first, int count) {
    if (!s->noise || !s->rn_v_on || count < 1) return TINYMPC_OK;
    const size_t at = (size_t)first * s->nx;
    HIP_TRY(hipMemcpyAsync(s->rn_px + at, s->dx0 + at, sizeof(double) * count * s->nx, hipMemcpyDeviceToDevice, s->stream));
    return TINYMPC_OK;
}

int tinympc_set_x0(tinympc_solver *s, const double *x0, int len, int verbose) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (!x0) return fail(TINYMPC_ERR_INVALID_INPUT, "set_x0: x0 is NULL");
    // The reference only perror()s on a wrong length and still assigns (tiny_api.cpp:238-241); an
    // Eigen column assignment of the wrong length is undefined behaviour, so the C ABI rejects it.
    if (len != s->nx) return fail(TINYMPC_ERR_INVALID_INPUT, "set_x0: x0 has %d entries, expected %d", len, s->nx);
    if (s->host_path()) {  // no device call at all: the next launch picks x0 up from pinned host memory
        // (a launch of tinympc_solve_async may still be reading the buffer: wait for it first)
        if (s->host_sol_state == 1 && (rc = tinympc_synchronize(s))) return rc;
        std::memcpy(s->h_x0, x0, sizeof(double) * s->nx);
        s->x0_on_host = true;
        if (verbose) printf("Initial state set\n");
        return TINYMPC_OK;
    }
    if ((rc = bind_device(s))) return rc;
    rc = upload(s, s->dx0, x0, s->nx);
    if (!rc) rc = mirror_x0_into_px(s, 0, 1);
    if (!rc && verbose) printf("Initial state set\n");
    return rc;
}

// tinympc_set_x_ref / tinympc_set_u_ref. keep_track: the call forwards the current window of a single-instance handle's reference
// track (forward_track_window below) -- the caller's own call ends the half's track mode.
static int set_x_ref_shared(tinympc_solver *s, const double *Xref, int rows, int cols, int verbose, bool keep_track) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (!Xref) return fail(TINYMPC_ERR_INVALID_INPUT, "set_x_ref: Xref is NULL");
    // The reference prints the mismatch and assigns anyway (tiny_api.cpp:250-254), which would change
    // the workspace shape under the solver; rejected here.
    if (rows != s->nx || cols != s->N)
        return fail(TINYMPC_ERR_INVALID_INPUT, "State reference trajectory (x_ref) is %d x %d. Expected %d x %d.", rows, cols, s->nx, s->N);
    s->inst.x = false;  // (per-instance references: this half is shared again, for every instance)
    if (!keep_track) { s->inst.x_track = false; s->inst.hXt.clear(); }  // (... and no longer a reference track)
    s->xref_const = rows_constant(Xref, s->nx, s->N);
    if (s->host_path()) {  // no device call: the next launch reads the pinned copy and rebuilds the table rows itself
        if (s->host_sol_state == 1 && (rc = tinympc_synchronize(s))) return rc;  // a launch in flight may be reading it
        const size_t col = sizeof(double) * s->nx;
        if (std::memcmp(s->h_xref, Xref, col * s->N) == 0) {
            // the same reference again (tracking loops re-send it every tick): nothing to do
        } else if (s->session_active && !s->refs_on_host && !s->xref_shift && std::memcmp(s->h_xref + s->nx, Xref, col * (s->N - 1)) == 0) {
            s->xref_shift = true;  // moved up by one knot: only the new last column has to travel
            std::memcpy(s->h_xref, Xref, col * s->N);
        } else {
            std::memcpy(s->h_xref, Xref, col * s->N);
            s->refs_on_host = true;
        }
        if (verbose) printf("State reference set\n");
        return TINYMPC_OK;
    }
    if ((rc = bind_device(s))) return rc;
    rc = upload(s, s->dXref, Xref, s->X());
    s->tables_dirty = true;
    if (!rc && verbose) printf("State reference set\n");
    return rc;
}
int tinympc_set_x_ref(tinympc_solver *s, const double *Xref, int rows, int cols, int verbose) {
    return set_x_ref_shared(s, Xref, rows, cols, verbose, false);
}

static int set_u_ref_shared(tinympc_solver *s, const double *Uref, int rows, int cols, int verbose, bool keep_track) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (!Uref) return fail(TINYMPC_ERR_INVALID_INPUT, "set_u_ref: Uref is NULL");
    if (rows != s->nu || cols != s->N - 1)
        return fail(TINYMPC_ERR_INVALID_INPUT, "Control/input reference trajectory (u_ref) is %d x %d. Expected %d x %d.", rows, cols, s->nu, s->N - 1);
    s->inst.u = false;
    if (!keep_track) { s->inst.u_track = false; s->inst.hUt.clear(); }
    s->uref_const = rows_constant(Uref, s->nu, s->N - 1);
    if (s->host_path()) {
        if (s->host_sol_state == 1 && (rc = tinympc_synchronize(s))) return rc;
        const size_t col = sizeof(double) * s->nu;
        if (std::memcmp(s->h_uref, Uref, col * (s->N - 1)) == 0) {
            // unchanged
        } else if (s->session_active && !s->refs_on_host && !s->uref_shift && s->N > 2 &&
                   std::memcmp(s->h_uref + s->nu, Uref, col * (s->N - 2)) == 0) {
            s->uref_shift = true;
            std::memcpy(s->h_uref, Uref, col * (s->N - 1));
        } else {
            std::memcpy(s->h_uref, Uref, col * (s->N - 1));
            s->refs_on_host = true;
        }
        if (verbose) printf("Input reference set\n");
        return TINYMPC_OK;
    }
    if ((rc = bind_device(s))) return rc;
    rc = upload(s, s->dUref, Uref, s->U());
    s->tables_dirty = true;
    if (!rc && verbose) printf("Input reference set\n");
    return rc;
}
int tinympc_set_u_ref(tinympc_solver *s, const double *Uref, int rows, int cols, int verbose) {
    return set_u_ref_shared(s, Uref, rows, cols, verbose, false);
}

int tinympc_set_bound_constraints(tinympc_solver *s, const double *x_min, const double *x_max,
                                  const double *u_min, const double *u_max, int verbose) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (!x_min || !x_max || !u_min || !u_max)
        return fail(TINYMPC_ERR_INVALID_INPUT, "set_bound_constraints requires x_min, x_max, u_min, u_max (expanded to nx x N / nu x (N-1))");
    if ((rc = bind_device(s))) return rc;
    if ((rc = upload(s, s->dxmin, x_min, s->X()))) return rc;
    if ((rc = upload(s, s->dxmax, x_max, s->X()))) return rc;
    if ((rc = upload(s, s->dumin, u_min, s->U()))) return rc;
    if ((rc = upload(s, s->dumax, u_max, s->U()))) return rc;
    s->xmin_const = rows_constant(x_min, s->nx, s->N); s->xmax_const = rows_constant(x_max, s->nx, s->N);
    s->umin_const = rows_constant(u_min, s->nu, s->N - 1); s->umax_const = rows_constant(u_max, s->nu, s->N - 1);
    s->st.en_state_bound = 1;  // bindings.cpp:206-207
    s->st.en_input_bound = 1;
    s->tables_dirty = true;
    s->inst.bounds = false;  // (per-instance bounds: every instance is on the shared bounds again)
    if (verbose) printf("Bound constraints set\n");
    return TINYMPC_OK;
}

int tinympc_solve_async(tinympc_solver *s) {
    int rc = check_handle(s);
    if (rc) return rc;
    if ((rc = bind_device(s))) return rc;
    return launch(s, false);
}

int tinympc_synchronize(tinympc_solver *s) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (s->session_active) return TINYMPC_OK;  // session steps are synchronous; the resident kernel never "finishes"
    if (s->flag_pending && s->host_sol_state == 1) {
        // The launch in flight raises a flag in pinned memory after its last store: poll it. Bounded: a kernel that takes
        // longer than the polling budget (long solves) is waited for the ordinary way.
        const volatile double *flag = s->h_sol + s->X() + s->U() + 6;
        const double want = (double)s->session_seq;
        for (int spin = 0; spin < 400000; ++spin) {
            if (*flag == want) {
                std::atomic_thread_fence(std::memory_order_acquire);
                s->flag_pending = false;
                s->host_sol_state = 2;
                s->dbg_tick[2] = (double)spin;
                s->dbg_tick[3] = 0.0;
                return TINYMPC_OK;
            }
            __builtin_ia32_pause();
        }
        s->dbg_tick[3] = 1.0;  // the polling budget ran out
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->flag_pending = false;
    if (s->host_sol_state == 1) s->host_sol_state = 2;
    return TINYMPC_OK;
}

// Resident solves (round 5, an extension; off by default): the reference's per-tick sequence  set_x0 -> solve -> get_solution  served by the
// resident session kernel instead of a launch per solve -- what tinympc_session_step does, behind the reference's own verbs, so that a
// script written against the reference needs ONE extra line (solver.set_resident(true)) for a 2.5x shorter tick. Bit-identical to
// launched solves (the session's contract). Everything that ends a session (any verb that needs the device) ends this one too; the next
// solve opens it again. Where no resident kernel exists for the configuration (batched handles, adaptive rho, wide systems) solves are
// launched as before.
int tinympc_set_resident(tinympc_solver *s, int enable) {
    int rc = check_handle(s);
    if (rc) return rc;
    s->resident_solves = enable != 0;
    s->resident_refused = false;
    if (!enable && s->session_active) {
        HIP_TRY(hipSetDevice(s->device));
        return end_session(s);
    }
    return TINYMPC_OK;
}

static int print_solve_result(tinympc_solver *s) {
    int it = 0, st = 0;
    int rc = tinympc_get_stats(s, &it, &st, nullptr, nullptr, 0);
    if (rc) return rc;
    if (st == TINYMPC_STATUS_SOLVED) printf("Solver converged in %d iterations\n", it);  // admm.cpp:190
    printf("Solve completed with status: %d\n", st == TINYMPC_STATUS_SOLVED ? 0 : 1);
    return TINYMPC_OK;
}

int tinympc_solve(tinympc_solver *s, int verbose) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (s->resident_solves && !s->resident_refused && s->host_path() && !s->inst.models) {  // (per-instance models: launched solves)
        if (!s->session_active) {
            rc = tinympc_session_begin(s);
            if (rc == TINYMPC_ERR_UNSUPPORTED || rc == TINYMPC_ERR_INVALID_INPUT) s->resident_refused = true;  // (launched solves from here on)
            else if (rc) return rc;
        }
        if (s->session_active) {
            double u0[16];
            if ((rc = tinympc_session_step(s, s->h_x0, u0))) return rc;  // (x0: what tinympc_set_x0 left in the pinned buffer)
            s->x0_on_host = false;
            return verbose ? print_solve_result(s) : TINYMPC_OK;
        }
    }
    rc = tinympc_solve_async(s);
    if (rc) return rc;
    if ((rc = tinympc_synchronize(s))) return rc;
    if (verbose) {
        int is[2] = {0, 0};
        if ((rc = download(s, is, s->distats, sizeof(is)))) return rc;
        if (is[1] == TINYMPC_STATUS_SOLVED) printf("Solver converged in %d iterations\n", is[0]);  // admm.cpp:190
        printf("Solve completed with status: %d\n", is[1] == TINYMPC_STATUS_SOLVED ? 0 : 1);
    }
    return TINYMPC_OK;
}

int tinympc_solve_timed(tinympc_solver *s, float *kernel_ms) {
    int rc = check_handle(s);
    if (rc) return rc;
    if ((rc = bind_device(s))) return rc;
    if ((rc = refresh_derived(s))) return rc;  // keep table rebuilds out of the timed region
    if ((rc = refresh_inst_tables(s))) return rc;
    if ((rc = launch(s, true))) return rc;
    HIP_TRY(hipEventSynchronize(s->ev1));
    if (s->host_sol_state == 1) s->host_sol_state = 2;
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, s->ev0, s->ev1));
    if (kernel_ms) *kernel_ms = ms;
    return TINYMPC_OK;
}

int tinympc_solve_queued(tinympc_solver *s) {
    int rc = check_handle(s);
    if (rc) return rc;
    if ((rc = bind_device(s))) return rc;
    if (s->session_active || s->host_path()) return fail(TINYMPC_ERR_UNSUPPORTED, "solve_queued: batched handles outside a session only");
    if (s->ring_count >= 4096) return fail(TINYMPC_ERR_INVALID_INPUT, "solve_queued: 4096 launches queued, collect their times first");
    if ((rc = refresh_derived(s))) return rc;  // keep table rebuilds out of the timed region
    if ((rc = refresh_inst_tables(s))) return rc;
    while ((int)s->ring_ev.size() < 2 * (s->ring_count + 1)) {
        hipEvent_t e = nullptr;
        HIP_TRY(hipEventCreate(&e));
        s->ring_ev.push_back(e);
    }
    // the launch records the handle's event pair: lend it this launch's slot of the ring
    hipEvent_t keep0 = s->ev0, keep1 = s->ev1;
    s->ev0 = s->ring_ev[2 * (size_t)s->ring_count];
    s->ev1 = s->ring_ev[2 * (size_t)s->ring_count + 1];
    rc = launch(s, true);
    s->ev0 = keep0;
    s->ev1 = keep1;
    if (rc) return rc;
    s->ring_count++;
    return TINYMPC_OK;
}

int tinympc_collect_kernel_ms(tinympc_solver *s, float *kernel_ms, int capacity, int *count) {
    int rc = check_handle(s);
    if (rc) return rc;
    if ((rc = bind_device(s))) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
    const int n = s->ring_count;
    if (count) *count = n;
    if (n > capacity || (n > 0 && !kernel_ms)) return fail(TINYMPC_ERR_INVALID_INPUT, "collect_kernel_ms: %d launches queued, room for %d", n, capacity);
    for (int i = 0; i < n; ++i) HIP_TRY(hipEventElapsedTime(&kernel_ms[i], s->ring_ev[2 * (size_t)i], s->ring_ev[2 * (size_t)i + 1]));
    s->ring_count = 0;
    return TINYMPC_OK;
}

static int advance_ref_steps_after_tick(tinympc_solver *s);  // (defined with the reference-track verbs below)

int tinympc_mpc_step_batch(tinympc_solver *s, const double *x0s, double *u0_out) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (!x0s || !u0_out) return fail(TINYMPC_ERR_INVALID_INPUT, "mpc_step: x0s and u0_out are required");
    if ((rc = bind_device(s))) return rc;
    const size_t nx0 = (size_t)s->batch * s->nx, nu0 = (size_t)s->batch * s->nu;
    s->x0_on_host = false;  // this call brings its own x0
    if (!s->h_x0) {  // pinned staging, so that the small copies are true async DMA and need no extra sync
        ArenaPlan pin;  // (one block for both; batched handles only -- a single-instance handle has them in its setup arena)
        pin.add(&s->h_x0, nx0); pin.add(&s->h_u0, nu0);
        void *base = nullptr;
        HIP_TRY(hipHostMalloc(&base, pin.mark(), hipHostMallocCoherent));
        s->host_allocs.push_back(base);
        pin.bind(base);
    }
    if (s->host_sol_state == 1) {  // a launch of tinympc_solve_async may still be reading h_x0
        HIP_TRY(hipStreamSynchronize(s->stream));
        s->host_sol_state = 2;
    }
    std::memcpy(s->h_x0, x0s, sizeof(double) * nx0);
    if ((rc = resolve_plan(s))) return rc;
    int zc_max = current_plan(s).layout == 'D' ? kZeroCopyTickMaxD : kZeroCopyTickMax;
    if (const char *e = getenv("TINYMPC_ZERO_COPY_MAX")) zc_max = atoi(e);  // (experiments)
    if (s->batch <= zc_max && s->st.max_iter > 0 && current_plan(s).host_exchange) {
        // Small batches: no copy engine at all. The kernel reads x0 from the pinned host buffer (and mirrors it into
        // the device copy the other verbs use) and writes the first controls into the pinned host buffer; both
        // are device-visible host allocations, and the stream synchronisation makes the writes visible here.
        s->zero_copy_tick = true;
        const auto t_a = std::chrono::steady_clock::now();
        rc = launch(s, false);
        const auto t_b = std::chrono::steady_clock::now();
        s->zero_copy_tick = false;
        if (rc) return rc;
        if ((rc = tinympc_synchronize(s))) return rc;  // (single instance: polls the completion flag in pinned memory)
        const auto t_c = std::chrono::steady_clock::now();
        s->dbg_tick[0] = std::chrono::duration<double, std::micro>(t_b - t_a).count();  // launch
        s->dbg_tick[1] = std::chrono::duration<double, std::micro>(t_c - t_b).count();  // wait
    } else {
        HIP_TRY(hipMemcpyAsync(s->dx0, s->h_x0, sizeof(double) * nx0, hipMemcpyHostToDevice, s->stream));
        if ((rc = launch(s, false))) return rc;
        HIP_TRY(hipMemcpy2DAsync(s->h_u0, sizeof(double) * s->nu, s->dsolu, sizeof(double) * s->U(), sizeof(double) * s->nu,
                                 s->batch, hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
    }
    std::memcpy(u0_out, s->h_u0, sizeof(double) * nu0);
    if ((rc = mirror_x0_into_px(s, 0, s->batch))) return rc;  // (this call brought its own x0: the true state restarts from it)
    // reference tracks: every step moves AFTER the tick's solve -- one small kernel behind it on the stream, nothing read back; the next
    // launch rebuilds the rows
    if (s->inst.auto_advance && (rc = advance_ref_steps_after_tick(s))) return rc;
    return TINYMPC_OK;
}




// ---- diagnostics (include/tinympc_hip_bench.h; not part of the drop-in boundary)
int tinympc_debug_setup_timing(tinympc_solver *s, double *out10) {
    int rc = check_handle(s);
    if (rc) return rc;
    for (int i = 0; i < 7; ++i) out10[i] = s->setup_us[i];
    int info[4] = {0, 0, 0, 0};
    if ((rc = bind_device(s))) return rc;
    if ((rc = download(s, info, s->dinfo, sizeof(info)))) return rc;
    out10[7] = (double)info[1];         // shader clocks of the Riccati loop (k_precompute_rows; 0 from the other precompute kernels)
    out10[8] = 0.01 * (double)info[2];  // ... its duration in us (100 MHz counter)
    out10[9] = (double)info[0];         // Riccati steps
    return TINYMPC_OK;
}

double tinympc_debug_mail_stamp(double sequence_number, const double *words7) { return tinympc::mail_stamp_of(sequence_number, words7); }

int tinympc_debug_tick_timing(tinympc_solver *s, double *out4) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (s->session_active && s->session_on_f && s->h_sol) {
        // layout F's resident kernel (not layout C's) leaves its own split of the last tick in the spare slot behind the completion stamp: us it waited
        // for the command since its previous answer, us of ADMM iterations, us of write-out (16 bits each, ticks of 10 ns)
        if (s->host_sol_state == 3 && (rc = wait_session_solution(s))) return rc;
        const unsigned long long packed = (unsigned long long)s->h_sol[s->X() + s->U() + 7];
        out4[0] = 0.01 * (double)(packed & 0xffffull);
        out4[1] = 0.01 * (double)((packed >> 16) & 0xffffull);
        out4[2] = 0.01 * (double)((packed >> 32) & 0xffffull);
        out4[3] = 0.0;
        return TINYMPC_OK;
    }
    for (int i = 0; i < 4; ++i) out4[i] = s->dbg_tick[i];
    return TINYMPC_OK;
}

int tinympc_get_solution_batch(tinympc_solver *s, double *x_out, double *u_out, int first, int count) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (first < 0 || count < 0 || first + count > s->batch)
        return fail(TINYMPC_ERR_INVALID_INPUT, "instance range [%d, %d) outside batch of %d", first, first + count, s->batch);
    if (s->host_path() && count == 1 && s->host_sol_state != 0) {
        if (s->host_sol_state == 1 && (rc = tinympc_synchronize(s))) return rc;
        if (s->host_sol_state == 3 && (rc = wait_session_solution(s))) return rc;
        if (x_out) std::memcpy(x_out, s->h_sol, sizeof(double) * s->X());
        if (u_out) std::memcpy(u_out, s->h_sol + s->X(), sizeof(double) * s->U());
        return TINYMPC_OK;
    }
    if ((rc = bind_device(s))) return rc;
    if ((rc = materialize_zero_solution(s))) return rc;
    if (x_out && (rc = download(s, x_out, s->dsolx + (size_t)first * s->X(), sizeof(double) * s->X() * count))) return rc;
    if (u_out && (rc = download(s, u_out, s->dsolu + (size_t)first * s->U(), sizeof(double) * s->U() * count))) return rc;
    return TINYMPC_OK;
}

int tinympc_get_solution(tinympc_solver *s, double *x_out, double *u_out, int verbose) {
    int rc = tinympc_get_solution_batch(s, x_out, u_out, 0, 1);
    if (!rc && verbose) printf("Solution retrieved\n");
    return rc;
}

int tinympc_get_first_controls_batch(tinympc_solver *s, double *u0_out, int first, int count) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (!u0_out) return fail(TINYMPC_ERR_INVALID_INPUT, "u0_out is NULL");
    if (first < 0 || count < 0 || first + count > s->batch)
        return fail(TINYMPC_ERR_INVALID_INPUT, "instance range [%d, %d) outside batch of %d", first, first + count, s->batch);
    if ((rc = bind_device(s))) return rc;
    if ((rc = materialize_zero_solution(s))) return rc;
    HIP_TRY(hipMemcpy2DAsync(u0_out, sizeof(double) * s->nu, s->dsolu + (size_t)first * s->U(), sizeof(double) * s->U(),
                             sizeof(double) * s->nu, count, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return TINYMPC_OK;
}

int tinympc_get_stats_batch(tinympc_solver *s, int *iters, int *status, double *residuals, int first, int count) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (first < 0 || count < 0 || first + count > s->batch)
        return fail(TINYMPC_ERR_INVALID_INPUT, "instance range [%d, %d) outside batch of %d", first, first + count, s->batch);
    if (s->host_path() && count == 1 && s->host_sol_state != 0) {
        if (s->host_sol_state == 1 && (rc = tinympc_synchronize(s))) return rc;
        if (s->host_sol_state == 3 && (rc = wait_session_solution(s))) return rc;
        const double *hs = s->h_sol + s->X() + s->U();
        if (iters) iters[0] = (int)hs[4];
        if (status) status[0] = (int)hs[5];
        if (residuals) std::memcpy(residuals, hs, sizeof(double) * 4);
        return TINYMPC_OK;
    }
    if ((rc = bind_device(s))) return rc;
    if (iters || status) {
        std::vector<int> is((size_t)count * 2);
        if ((rc = download(s, is.data(), s->distats + (size_t)first * 2, sizeof(int) * 2 * count))) return rc;
        for (int b = 0; b < count; ++b) {
            if (iters) iters[b] = is[2 * (size_t)b];
            if (status) status[b] = is[2 * (size_t)b + 1];
        }
    }
    if (residuals && (rc = download(s, residuals, s->ddstats + (size_t)first * 4, sizeof(double) * 4 * count))) return rc;
    return TINYMPC_OK;
}

int tinympc_get_stats(tinympc_solver *s, int *iter, int *status, double *pri_res_state, double *pri_res_input, int verbose) {
    double res[4];
    int it = 0, st = 0;
    int rc = tinympc_get_stats_batch(s, &it, &st, res, 0, 1);
    if (rc) return rc;
    if (iter) *iter = it;
    if (status) *status = st;
    if (pri_res_state) *pri_res_state = res[0];
    if (pri_res_input) *pri_res_input = res[2];
    if (verbose) printf("Statistics retrieved: iter=%d, status=%d\n", it, st);
    return TINYMPC_OK;
}

int tinympc_get_residuals(tinympc_solver *s, double residuals[4]) {
    return tinympc_get_stats_batch(s, nullptr, nullptr, residuals, 0, 1);
}

namespace {
// Gather what the emitter needs from the device (the cache the kernels computed or the caller installed, the
// rho-augmented cost diagonals, dynamics, bounds) and write the embedded project's data files.
int codegen_from_handle(tinympc_solver *s, const char *output_dir, const double *dK, const double *dP, const double *dC1,
                        const double *dC2, int verbose) {
    int rc = bind_device(s);
    if (rc) return rc;
    const size_t nx = s->nx, nu = s->nu, X = s->X(), U = s->U();
    std::vector<double> K(nu * nx), P(nx * nx), Qi(nu * nu), Am(nx * nx), qd(nx), rd(nu), A(nx * nx), B(nx * nu), xmin(X), xmax(X), umin(U), umax(U);
    const struct { void *dst; const void *src; size_t n; } pulls[] = {
        {K.data(), s->dKinf, K.size()}, {P.data(), s->dPinf, P.size()}, {Qi.data(), s->dQuu, Qi.size()}, {Am.data(), s->dAmBKt, Am.size()},
        {qd.data(), s->dQd, nx}, {rd.data(), s->dRd, nu}, {A.data(), s->dA, A.size()}, {B.data(), s->dB, B.size()},
        {xmin.data(), s->dxmin, X}, {xmax.data(), s->dxmax, X}, {umin.data(), s->dumin, U}, {umax.data(), s->dumax, U}};
    for (const auto &p : pulls)
        if ((rc = download(s, p.dst, p.src, sizeof(double) * p.n))) return rc;
    int is[2] = {0, 0};  // iter, status of instance 0
    if ((rc = download(s, is, s->distats, sizeof(is)))) return rc;
    tinympc_codegen_data d{};
    d.nx = s->nx; d.nu = s->nu; d.N = s->N; d.rho = s->rho;
    d.iter = is[0]; d.solved = is[1] == TINYMPC_STATUS_SOLVED ? 1 : 0;
    d.Kinf = K.data(); d.Pinf = P.data(); d.Quu_inv = Qi.data(); d.AmBKt = Am.data();
    d.dKinf_drho = dK; d.dPinf_drho = dP; d.dC1_drho = dC1; d.dC2_drho = dC2;
    d.abs_pri_tol = s->st.abs_pri_tol; d.abs_dua_tol = s->st.abs_dua_tol; d.max_iter = s->st.max_iter;
    d.check_termination = s->st.check_termination; d.en_state_bound = s->st.en_state_bound; d.en_input_bound = s->st.en_input_bound;
    d.adaptive_rho = s->st.adaptive_rho;
    d.Q = qd.data(); d.R = rd.data(); d.Adyn = A.data(); d.Bdyn = B.data();
    d.x_min = xmin.data(); d.x_max = xmax.data(); d.u_min = umin.data(); d.u_max = umax.data();
    return tinympc_codegen_emit(&d, output_dir, verbose);
}
}  // namespace

int tinympc_codegen(tinympc_solver *s, const char *output_dir, int verbose) {
    int rc = check_handle(s);
    if (rc) return rc;
    return codegen_from_handle(s, output_dir, nullptr, nullptr, nullptr, nullptr, verbose);
}

int tinympc_codegen_with_sensitivity(tinympc_solver *s, const char *output_dir, const double *dK, const double *dP, const double *dC1,
                                     const double *dC2, int verbose) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (!dK || !dP || !dC1 || !dC2) return fail(TINYMPC_ERR_INVALID_INPUT, "codegen_with_sensitivity requires dK, dP, dC1, dC2");
    // the four matrices reach the cache (and the generated file) only while adaptive_rho is enabled (codegen.cpp:79-86, 237-252)
    if (s->st.adaptive_rho) {
        if ((rc = bind_device(s))) return rc;
        if ((rc = upload(s, s->ddK, dK, (size_t)s->nu * s->nx))) return rc;
        if ((rc = upload(s, s->ddP, dP, (size_t)s->nx * s->nx))) return rc;
    }
    return codegen_from_handle(s, output_dir, dK, dP, dC1, dC2, verbose);
}

int tinympc_set_sensitivity_matrices(tinympc_solver *s, const double *dK, const double *dP, const double *dC1, const double *dC2, int verbose) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (!dK || !dP || !dC1 || !dC2) return fail(TINYMPC_ERR_INVALID_INPUT, "set_sensitivity_matrices requires 4 matrices");
    // bindings.cpp:338-352 only prints their norms; the old core's adaptive-rho update reads them from the cache
    // (rho_benchmark.cpp:205-208), which is where they go here: dKinf/drho and dPinf/drho feed k_admm_solve_adapt
    // (dC1/dC2 would update C1/C2, which no solve phase reads).
    if ((rc = bind_device(s))) return rc;
    if ((rc = upload(s, s->ddK, dK, (size_t)s->nu * s->nx))) return rc;
    if ((rc = upload(s, s->ddP, dP, (size_t)s->nx * s->nx))) return rc;
    if (verbose) printf("Sensitivity matrices set\n");
    return TINYMPC_OK;
}

int tinympc_set_cache_terms(tinympc_solver *s, const double *Kinf, const double *Pinf, const double *Quu_inv, const double *AmBKt, int verbose) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (!Kinf || !Pinf || !Quu_inv || !AmBKt) return fail(TINYMPC_ERR_INVALID_INPUT, "set_cache_terms requires Kinf, Pinf, Quu_inv, AmBKt");
    if ((rc = bind_device(s))) return rc;
    if ((rc = upload(s, s->dKinf, Kinf, (size_t)s->nu * s->nx))) return rc;
    if ((rc = upload(s, s->dPinf, Pinf, (size_t)s->nx * s->nx))) return rc;
    if ((rc = upload(s, s->dQuu, Quu_inv, (size_t)s->nu * s->nu))) return rc;
    if ((rc = upload(s, s->dAmBKt, AmBKt, (size_t)s->nx * s->nx))) return rc;
    s->ops_dirty = true;
    s->tables_dirty = true;
    if (verbose) printf("Cache terms set\n");
    return TINYMPC_OK;
}

int tinympc_set_linear_constraints(tinympc_solver *s, const double *Alin_x, const double *blin_x, int nlx,
                                   const double *Alin_u, const double *blin_u, int nlu) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (nlx < 0 || nlu < 0) return fail(TINYMPC_ERR_INVALID_INPUT, "negative constraint count");
    if ((nlx > 0 && (!Alin_x || !blin_x)) || (nlu > 0 && (!Alin_u || !blin_u)))
        return fail(TINYMPC_ERR_INVALID_INPUT, "set_linear_constraints: NULL matrix for a non-empty side");
    if (s->session_active && (rc = bind_device(s))) return rc;  // the resident kernel was started with the old families
    // (up to MAX_LIN_ROWS rows per side every kernel holds; beyond, the structure-specialised kernels -- layouts E and F -- size
    // their copies from the count itself: checked at launch, where the kernel is known)
    if (nlx > HARD_MAX_LIN_ROWS || nlu > HARD_MAX_LIN_ROWS)
        return fail(TINYMPC_ERR_UNSUPPORTED, "at most %d linear rows per side are supported by the HIP kernels (got %d state, %d input)",
                    HARD_MAX_LIN_ROWS, nlx, nlu);
    auto zero_row = [](const double *A, int rows, int cols, int k) {
        for (int c = 0; c < cols; ++c)
            if (A[k + (size_t)c * rows] != 0.0) return false;
        return true;
    };
    for (int k = 0; k < nlx; ++k)
        if (zero_row(Alin_x, nlx, s->nx, k)) return fail(TINYMPC_ERR_INVALID_INPUT, "Alin_x row %d is all zero", k);
    for (int k = 0; k < nlu; ++k)
        if (zero_row(Alin_u, nlu, s->nu, k)) return fail(TINYMPC_ERR_INVALID_INPUT, "Alin_u row %d is all zero", k);
    if (s->inst.lin) {  // (per-instance linear rows, per knot too: every instance is on the shared rows again)
        s->inst.lin = false;
        s->inst.lin_knots = 0;
        if (s->inst_tables()) s->inst.mark(0, s->batch);
    }
    s->inst.shared_rows_dirty = true;  // (per-instance cone slopes alone: the store's rows are a copy of these)
    s->n_lin_x = nlx;
    s->n_lin_u = nlu;
    s->Alin_x.assign(Alin_x, Alin_x + (size_t)nlx * s->nx);
    s->blin_x.assign(blin_x, blin_x + nlx);
    s->Alin_u.assign(Alin_u, Alin_u + (size_t)nlu * s->nu);
    s->blin_u.assign(blin_u, blin_u + nlu);
    if (nlx > 0) s->st.en_state_linear = 1;  // bindings.cpp:422-429
    if (nlu > 0) s->st.en_input_linear = 1;
    s->fam_dirty = true;
    return TINYMPC_OK;
}

int tinympc_set_cone_constraints(tinympc_solver *s, const int *Acx, const int *qcx, const double *cx, int ncx,
                                 const int *Acu, const int *qcu, const double *cu, int ncu) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (ncx < 0 || ncu < 0) return fail(TINYMPC_ERR_INVALID_INPUT, "negative cone count");
    if ((ncx > 0 && (!Acx || !qcx || !cx)) || (ncu > 0 && (!Acu || !qcu || !cu)))
        return fail(TINYMPC_ERR_INVALID_INPUT, "set_cone_constraints: NULL array for a non-empty side");
    if (s->session_active && (rc = bind_device(s))) return rc;  // the resident kernel was started with the old families
    // Each cone must lie inside its vector. Cones of one side MAY share rows: upstream projects the cones of a knot one after
    // another (bindings.cpp:433-478 hands the list over in order), which the kernels reproduce by grouping the list into rounds of
    // pairwise-disjoint cones (family_structure). Up to MAX_CONES cones in MAX_ROUNDS rounds every families kernel holds; up to
    // HARD_MAX_CONES in any number of rounds run on the structure-specialised kernels (layouts E and F).
    auto check_side = [&](const int *Ac, const int *qc, const double *c, int n, int dim, const char *side) -> int {
        for (int k = 0; k < n; ++k) {
            if (qc[k] < 1 || Ac[k] < 0 || Ac[k] + qc[k] > dim)
                return fail(TINYMPC_ERR_INVALID_INPUT, "%s cone %d (start %d, dimension %d) does not fit a vector of %d rows", side, k, Ac[k], qc[k], dim);
            if (!(c[k] > 0.0)) return fail(TINYMPC_ERR_INVALID_INPUT, "%s cone %d has non-positive slope %g", side, k, c[k]);
        }
        return TINYMPC_OK;
    };
    if ((rc = check_side(Acx, qcx, cx, ncx, s->nx, "state"))) return rc;
    if ((rc = check_side(Acu, qcu, cu, ncu, s->nu, "input"))) return rc;
    if (ncx + ncu > HARD_MAX_CONES)
        return fail(TINYMPC_ERR_UNSUPPORTED, "at most %d cones are supported by the HIP kernels (got %d state + %d input)", HARD_MAX_CONES, ncx, ncu);
    {   // rounds of the whole list, both sides enabled (the worst case of what a launch can see)
        int rounds = 0;
        unsigned long long used = 0;
        auto walk = [&](const int *Ac, const int *qc, int n, int base) {
            for (int k = 0; k < n; ++k) {
                unsigned long long lanes = 0;
                for (int r = base + Ac[k]; r < base + Ac[k] + qc[k]; ++r) lanes |= 1ull << (r & 63);
                if (rounds == 0) rounds = 1;
                if (lanes & used) {
                    rounds += 1;
                    used = 0;
                }
                used |= lanes;
            }
        };
        if (s->nx + s->nu <= 64) {  // (larger systems: layout M walks the cone list in order, it has no rounds)
            walk(Acx, qcx, ncx, 0);
            walk(Acu, qcu, ncu, s->nx);
        }
        // (more than MAX_ROUNDS rounds, like more than MAX_CONES cones: the structure-specialised kernels only -- checked at launch)
        (void)rounds;
    }
    s->n_cone_x = ncx;
    s->n_cone_u = ncu;
    s->Acx.assign(Acx, Acx + ncx); s->qcx.assign(qcx, qcx + ncx); s->cx.assign(cx, cx + ncx);
    s->Acu.assign(Acu, Acu + ncu); s->qcu.assign(qcu, qcu + ncu); s->cu.assign(cu, cu + ncu);
    if (s->inst.cones) {  // (per-instance cone slopes: a new structure, every instance on the shared slopes again)
        s->inst.cones = false;
        if (s->inst_tables()) s->inst.mark(0, s->batch);
    }
    s->inst.slopes_dirty = true;  // (per-instance linear rows alone: the store's slope vectors are a copy of these)
    if (ncx > 0) s->st.en_state_soc = 1;  // bindings.cpp:468-476
    if (ncu > 0) s->st.en_input_soc = 1;
    s->fam_dirty = true;
    return TINYMPC_OK;
}

int tinympc_reset(tinympc_solver **s, int verbose) {
    if (!s || !*s) return TINYMPC_OK;  // bindings.cpp:539: silently nothing to do
    destroy(*s);
    *s = nullptr;
    if (verbose) printf("Solver reset\n");
    return TINYMPC_OK;
}

int tinympc_update_settings(tinympc_solver *s, double abs_pri_tol, double abs_dua_tol, int max_iter, int check_termination,
                            int en_state_bound, int en_input_bound, int en_state_soc, int en_input_soc,
                            int en_state_linear, int en_input_linear, int adaptive_rho, double adaptive_rho_min,
                            double adaptive_rho_max, int adaptive_rho_enable_clipping, int verbose) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (max_iter < 0) return fail(TINYMPC_ERR_INVALID_INPUT, "max_iter must be >= 0");
    // A resident session kernel carries the settings it was launched with (max_iter, tolerances, family flags): end it, so
    // that nothing switches behaviour in the middle of a session or bypasses the checks of tinympc_session_begin on a
    // restart after the idle time-out. The next tinympc_session_begin starts one with the new settings.
    if (s->session_active && (rc = bind_device(s))) return rc;
    const bool bounds_changed = (s->st.en_state_bound != en_state_bound) || (s->st.en_input_bound != en_input_bound);
    s->st.abs_pri_tol = abs_pri_tol; s->st.abs_dua_tol = abs_dua_tol;
    s->st.max_iter = max_iter; s->st.check_termination = check_termination;
    s->st.en_state_bound = en_state_bound; s->st.en_input_bound = en_input_bound;
    // (the cones' rounds follow the enabled sides, and the per-instance slope vectors the rounds)
    if ((s->st.en_state_soc != 0) != (en_state_soc != 0) || (s->st.en_input_soc != 0) != (en_input_soc != 0)) s->inst.slopes_dirty = true;
    s->st.en_state_soc = en_state_soc; s->st.en_input_soc = en_input_soc;
    s->st.en_state_linear = en_state_linear; s->st.en_input_linear = en_input_linear;
    s->st.adaptive_rho = adaptive_rho; s->st.adaptive_rho_min = adaptive_rho_min;
    s->st.adaptive_rho_max = adaptive_rho_max; s->st.adaptive_rho_enable_clipping = adaptive_rho_enable_clipping;
    if (bounds_changed) s->tables_dirty = true;
    s->fam_dirty = true;  // the family enable flags are folded into the per-lane family description
    if (verbose) printf("Settings updated successfully\n");
    return TINYMPC_OK;
}

int tinympc_print_problem_data(tinympc_solver *s) {
    int rc = check_handle(s);
    if (rc) return rc;
    int is[2] = {0, 0};
    if ((rc = bind_device(s))) return rc;
    if ((rc = download(s, is, s->distats, sizeof(is)))) return rc;
    printf("solution iter: %d\nsolution solved: %d\n", is[0], is[1] == TINYMPC_STATUS_SOLVED);
    printf("\n\ncache rho: %f\n", s->rho);
    printf("\n\nabs_pri_tol: %f\nabs_dua_tol: %f\nmax_iter: %d\ncheck_termination: %d\nen_state_bound: %d\nen_input_bound: %d\n",
           s->st.abs_pri_tol, s->st.abs_dua_tol, s->st.max_iter, s->st.check_termination, s->st.en_state_bound, s->st.en_input_bound);
    printf("\n\nnx: %d\nnu: %d\niter: %d\nstatus: %d\n", s->nx, s->nu, is[0], is[1]);
    return TINYMPC_OK;
}

int tinympc_get_cache(tinympc_solver *s, double *Kinf, double *Pinf, double *Quu_inv, double *AmBKt, int *riccati_iters) {
    int rc = check_handle(s);
    if (rc) return rc;
    if ((rc = bind_device(s))) return rc;
    if (Kinf && (rc = download(s, Kinf, s->dKinf, sizeof(double) * s->nu * s->nx))) return rc;
    if (Pinf && (rc = download(s, Pinf, s->dPinf, sizeof(double) * s->nx * s->nx))) return rc;
    if (Quu_inv && (rc = download(s, Quu_inv, s->dQuu, sizeof(double) * s->nu * s->nu))) return rc;
    if (AmBKt && (rc = download(s, AmBKt, s->dAmBKt, sizeof(double) * s->nx * s->nx))) return rc;
    if (riccati_iters && (rc = download(s, riccati_iters, s->dinfo, sizeof(int)))) return rc;
    return TINYMPC_OK;
}

namespace {
// One Riccati recursion of the .m class on the device; results land in slot `slot` of dlqr_out.
int run_lqr(tinympc_solver *s, int slot, double rho, double reg, double tol, int norm_kind, int max_iter, int min_iter, int p0_augmented) {
    LqrParams p{};
    p.nx = s->nx; p.nu = s->nu; p.rho = rho; p.reg = reg; p.tol = tol; p.norm_kind = norm_kind;
    p.max_iter = max_iter; p.min_iter = min_iter; p.p0_augmented = p0_augmented;
    p.A = s->dA; p.B = s->dB; p.Q = s->dQfull; p.R = s->dRfull;
    double *o = s->dlqr_out + (size_t)slot * s->cache_doubles();
    p.K = o; p.P = p.K + (size_t)s->nu * s->nx; p.C1 = p.P + (size_t)s->nx * s->nx; p.C2 = p.C1 + (size_t)s->nu * s->nu;
    p.info = s->dinfo + 1 + slot; p.scratch = s->dlqr_scratch;
    p.use_lds = lqr_scratch_doubles(s->nx, s->nu) <= 6500 ? 1 : 0;
    HIP_TRY(launch_lqr(p, s->stream));
    return TINYMPC_OK;
}

int download_cache_slot(tinympc_solver *s, int slot, double *K, double *P, double *C1, double *C2) {
    const double *o = s->dlqr_out + (size_t)slot * s->cache_doubles();
    const size_t nK = (size_t)s->nu * s->nx, nP = (size_t)s->nx * s->nx, nC1 = (size_t)s->nu * s->nu;
    int rc;
    if (K && (rc = download(s, K, o, sizeof(double) * nK))) return rc;
    if (P && (rc = download(s, P, o + nK, sizeof(double) * nP))) return rc;
    if (C1 && (rc = download(s, C1, o + nK + nP, sizeof(double) * nC1))) return rc;
    if (C2 && (rc = download(s, C2, o + nK + nP + nC1, sizeof(double) * nP))) return rc;
    return TINYMPC_OK;
}
}  // namespace

// TinyMPC.m:194-221: P0 = Q, up to 5000 steps, 1e-8 regulariser in the gain solve, stop at norm(K-Kprev) < 1e-10.
int tinympc_compute_cache_terms(tinympc_solver *s, double *Kinf, double *Pinf, double *Quu_inv, double *AmBKt, int *iters, int verbose) {
    int rc = check_handle(s);
    if (rc) return rc;
    if ((rc = bind_device(s))) return rc;
    if ((rc = run_lqr(s, 0, s->rho, 1e-8, 1e-10, 2, 5000, 1, 0))) return rc;
    if ((rc = download_cache_slot(s, 0, Kinf, Pinf, Quu_inv, AmBKt))) return rc;
    int it = 0;
    if ((rc = download(s, &it, s->dinfo + 1, sizeof(int)))) return rc;
    if (iters) *iters = it;
    if (verbose) printf("Cache terms computed on the device after %d Riccati steps\n", it);
    return TINYMPC_OK;
}

// TinyMPC.m:336-366: the stabilising solution of the DARE for Q + rho I, R + rho I (MATLAB: idare; here the same
// fixed-point recursion as the class's fallback branch, without regulariser, run until K stops changing).
int tinympc_solve_lqr(tinympc_solver *s, double rho_val, double *K, double *P, double *C1, double *C2, int *iters) {
    int rc = check_handle(s);
    if (rc) return rc;
    if ((rc = bind_device(s))) return rc;
    if ((rc = run_lqr(s, 0, rho_val, 0.0, 1e-15, 0, 200000, 2, 1))) return rc;
    if ((rc = download_cache_slot(s, 0, K, P, C1, C2))) return rc;
    if (iters && (rc = download(s, iters, s->dinfo + 1, sizeof(int)))) return rc;
    return TINYMPC_OK;
}

// TinyMPC.m:223-241: forward differences of solve_lqr in rho with h = 1e-6.
int tinympc_compute_sensitivity(tinympc_solver *s, double *dK, double *dP, double *dC1, double *dC2, int verbose) {
    int rc = check_handle(s);
    if (rc) return rc;
    if ((rc = bind_device(s))) return rc;
    const double h = 1e-6;
    if ((rc = run_lqr(s, 0, s->rho, 0.0, 1e-15, 0, 200000, 2, 1))) return rc;
    if ((rc = run_lqr(s, 1, s->rho + h, 0.0, 1e-15, 0, 200000, 2, 1))) return rc;
    FiniteDiffParams f{};
    f.count = (int)s->cache_doubles(); f.h = h;
    f.lo = s->dlqr_out; f.hi = s->dlqr_out + s->cache_doubles(); f.out = s->dlqr_out + 2 * s->cache_doubles();
    HIP_TRY(launch_finite_diff(f, s->stream));
    if ((rc = download_cache_slot(s, 2, dK, dP, dC1, dC2))) return rc;
    if (verbose) printf("Sensitivity matrices computed on the device (forward differences, h = %g)\n", h);
    return TINYMPC_OK;
}

int tinympc_set_x0_batch(tinympc_solver *s, const double *x0s, int first, int count) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (!x0s) return fail(TINYMPC_ERR_INVALID_INPUT, "x0s is NULL");
    if (first < 0 || count < 0 || first + count > s->batch)
        return fail(TINYMPC_ERR_INVALID_INPUT, "instance range [%d, %d) outside batch of %d", first, first + count, s->batch);
    if ((rc = bind_device(s))) return rc;
    if (s->host_path() && count == 1) {
        // A single-instance handle keeps x0 twice: dx0 for launches, the pinned h_x0 for resident solves (tinympc_solve hands it to the
        // session) -- this verb brings BOTH up to date, as tinympc_set_x0 does through the kernel's mirror. (A launch of
        // tinympc_solve_async may still be reading the pinned buffer: wait for it first, as tinympc_set_x0 does.)
        if (s->host_sol_state == 1 && (rc = tinympc_synchronize(s))) return rc;
        std::memcpy(s->h_x0, x0s, sizeof(double) * s->nx);
    }
    s->x0_on_host = false;
    if ((rc = upload(s, s->dx0 + (size_t)first * s->nx, x0s, (size_t)count * s->nx))) return rc;
    return mirror_x0_into_px(s, first, count);
}

int tinympc_set_x0_batch_device(tinympc_solver *s, const double *d_x0s, int first, int count) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (!d_x0s) return fail(TINYMPC_ERR_INVALID_INPUT, "d_x0s is NULL");
    if (first < 0 || count < 0 || first + count > s->batch)
        return fail(TINYMPC_ERR_INVALID_INPUT, "instance range [%d, %d) outside batch of %d", first, first + count, s->batch);
    if ((rc = bind_device(s))) return rc;
    s->x0_on_host = false;
    HIP_TRY(hipMemcpyAsync(s->dx0 + (size_t)first * s->nx, d_x0s, sizeof(double) * count * s->nx, hipMemcpyDeviceToDevice, s->stream));
    if ((rc = mirror_x0_into_px(s, first, count))) return rc;
    // (a single-instance handle: the pinned copy that resident solves read follows on the same stream, behind any launch still reading it)
    if (s->host_path() && count == 1) HIP_TRY(hipMemcpyAsync(s->h_x0, s->dx0, sizeof(double) * s->nx, hipMemcpyDeviceToHost, s->stream));
    // The copy runs on the handle's own (non-blocking) stream: wait for it here, so that the caller may free or reuse
    // d_x0s as soon as the call returns -- the same ownership rule as every host-pointer verb. (Work that PRODUCES
    // d_x0s on another stream must have completed before the call; see the header.)
    HIP_TRY(hipStreamSynchronize(s->stream));
    return TINYMPC_OK;
}

namespace {

// `p` is device memory of the handle's own GPU (a host pointer or another GPU's memory is not)
bool on_handles_device(const tinympc_solver *s, const void *p) {
    hipPointerAttribute_t attr{};
    const hipError_t e = hipPointerGetAttributes(&attr, p);
    (void)hipGetLastError();
    return e == hipSuccess && attr.type == hipMemoryTypeDevice && attr.device == s->device;
}

// One array of a per-instance verb: the handle's rows x cols block per instance, and where it goes.
struct InstArray {
    const double *src;      // the caller's blocks, one per instance: rows x cols, or rows x 1 (one column held over the horizon)
    int rows, cols;
    double **store;         // the per-instance store [batch][cols][rows] (InstState; alloc_inst_state)
    const double *shared;   // what every instance holds when the mode begins ...
    bool shared_const;      // ... and whether that is constant over the horizon
    bool *constant;         // the mode's "constant over the horizon" flag (NULL: the caller keeps it -- reference tracks)
};

// The per-instance stores of `a`, the table rows (SolveParams::iref_lr / iref_pn / ibnd) and, for the bounds, layout A's clamp rows:
// allocated at the first per-instance verb that needs them.
int alloc_inst_state(tinympc_solver *s, const InstArray *a, int n, bool bounds) {
    const InstState &in = s->inst;
    int rc;
    for (int i = 0; i < n; ++i)
        if (!*a[i].store && (rc = dalloc(s, a[i].store, (size_t)a[i].rows * a[i].cols * s->batch))) return rc;
    return alloc_inst_rows(s, bounds || in.models);
}

// The one upload path of the per-instance verbs: arrays a[0, n) of instances [first, first+count), per knot or one column each
// (one_col). The mode enters at its first call (every instance then holds the shared value of that moment); the table rows of the
// instances named here are rebuilt at the next launch (refresh_inst_tables). Single-instance handles: `shared_verb`, handed the arrays
// expanded to rows x cols. `verb` names the range error, `dev_verb` / `noun` the device-memory one.
int set_inst_batch(tinympc_solver *s, const char *verb, const char *dev_verb, const char *noun, const InstArray *a, int n, bool &mode,
                   bool bounds, bool on_device, bool one_col, int first, int count, int (*shared_verb)(tinympc_solver *, const double *const *)) {
    int rc;
    if (first < 0 || count < 0 || first + count > s->batch)
        return fail(TINYMPC_ERR_INVALID_INPUT, "%s: instance range [%d, %d) outside batch of %d", verb, first, first + count, s->batch);
    for (int i = 0; on_device && count > 0 && i < n; ++i) {  // device memory of the handle's own GPU (a host pointer or another GPU's memory is refused here)
        hipPointerAttribute_t attr{};
        const hipError_t e = hipPointerGetAttributes(&attr, a[i].src);
        (void)hipGetLastError();
        if (e != hipSuccess || attr.type != hipMemoryTypeDevice || attr.device != s->device)
            return fail(TINYMPC_ERR_INVALID_INPUT, "%s: the %s are not device memory of the handle's GPU %d", dev_verb, noun, s->device);
    }
    if (s->batch == 1) {  // the shared verb, pinned-host path included
        if (count == 0) return TINYMPC_OK;
        if (on_device && (rc = bind_device(s))) return rc;
        std::vector<double> h[4];
        const double *hp[4];
        for (int i = 0; i < n; ++i) {
            const size_t per = (size_t)a[i].rows * a[i].cols, in_per = one_col ? (size_t)a[i].rows : per;
            std::vector<double> in;
            const double *src = a[i].src;
            if (on_device) {
                in.resize(in_per);
                if ((rc = download(s, in.data(), src, sizeof(double) * in_per))) return rc;
                src = in.data();
            }
            h[i].resize(per);
            for (size_t e = 0; e < per; ++e) h[i][e] = src[one_col ? e % a[i].rows : e];
            hp[i] = h[i].data();
        }
        return shared_verb(s, hp);
    }
    if ((rc = bind_device(s))) return rc;
    if (bounds && (!s->st.en_state_bound || !s->st.en_input_bound)) {  // like the shared verb, bindings.cpp:206-207
        s->st.en_state_bound = 1;
        s->st.en_input_bound = 1;
        s->tables_dirty = true;  // (the shared tables follow the flags; refresh_derived then marks every instance's rows)
    }
    if (s->layout_m) {  // (no kernel carries them: the next launch refuses until the shared verb clears the mode)
        mode = true;
        return TINYMPC_OK;
    }
    if ((rc = alloc_inst_state(s, a, n, bounds))) return rc;
    if (!mode) {  // every instance starts from the shared value of this moment
        for (int i = 0; i < n; ++i) *a[i].constant = true;
        for (int i = 0; i < n; ++i) {
            InstRefStoreParams b{};
            b.src = a[i].shared; b.src_stride = 0; b.rows = a[i].rows; b.src_cols = a[i].cols; b.cols = a[i].cols;
            b.first = 0; b.count = s->batch; b.dst = *a[i].store;
            HIP_TRY(launch_store_inst_refs(b, s->stream));
            *a[i].constant = *a[i].constant && a[i].shared_const;
        }
        mode = true;
        s->inst.mark(0, s->batch);
    }
    if (count > 0) {
        for (int i = 0; i < n; ++i) {
            const int R = a[i].rows, C = a[i].cols;
            const size_t per = (size_t)R * C;
            if (!one_col) {  // per knot: the caller's layout is the handle's
                bool constant = !on_device && a[i].constant;  // (device input: not looked at; reference tracks: never constant)
                for (int b = 0; constant && b < count; ++b) constant = rows_constant(a[i].src + (size_t)b * per, R, C);
                if (!constant && a[i].constant) *a[i].constant = false;
                HIP_TRY(hipMemcpyAsync(*a[i].store + (size_t)first * per, a[i].src, sizeof(double) * per * count,
                                       on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s->stream));
            } else {  // one column: held over the horizon on the device
                const double *dsrc = a[i].src;
                if (!on_device) {
                    const size_t cap = (size_t)s->batch * (s->nx > s->nu ? s->nx : s->nu);
                    if (!s->inst.stage && (rc = dalloc(s, &s->inst.stage, cap))) return rc;
                    HIP_TRY(hipMemcpyAsync(s->inst.stage, a[i].src, sizeof(double) * R * count, hipMemcpyHostToDevice, s->stream));
                    dsrc = s->inst.stage;
                }
                InstRefStoreParams b{};
                b.src = dsrc; b.src_stride = R; b.rows = R; b.src_cols = 1; b.cols = C;
                b.first = first; b.count = count; b.dst = *a[i].store;
                HIP_TRY(launch_store_inst_refs(b, s->stream));
            }
        }
        s->inst.mark(first, first + count);
    }
    // the caller keeps ownership of its buffers: the copies have completed when the call returns (the tinympc_set_x0_batch_device rule)
    HIP_TRY(hipStreamSynchronize(s->stream));
    return TINYMPC_OK;
}

// tinympc_set_x_ref_batch / _u_ref_batch (+ _device): one half (x or u) of the references, a goal (cols = 1) or a trajectory per instance.
int set_ref_batch(tinympc_solver *s, bool is_x, const double *src, bool on_device, int rows, int cols, int first, int count) {
    const char *verb = is_x ? "set_x_ref_batch" : "set_u_ref_batch";
    int rc = check_handle(s);
    if (rc) return rc;
    if (!src) return fail(TINYMPC_ERR_INVALID_INPUT, "%s: references are NULL", verb);
    const int R = is_x ? s->nx : s->nu, C = is_x ? s->N : s->N - 1;
    if (rows != R || (cols != C && cols != 1))
        return fail(TINYMPC_ERR_INVALID_INPUT, "%s: the references are %d x %d per instance. Expected %d x %d or %d x 1.", verb, rows, cols, R, C, R);
    InstState &in = s->inst;
    bool &track = is_x ? in.x_track : in.u_track;
    if (track && s->batch > 1) {  // a half in track mode: a whole-batch call returns it to plain per-instance references
        if (first != 0 || count != s->batch)
            return fail(TINYMPC_ERR_INVALID_INPUT, "%s: this half holds a reference track: name the whole batch (first = 0, count = %d) to replace it "
                        "with per-instance references", verb, s->batch);
        if (on_device && !on_handles_device(s, src))
            return fail(TINYMPC_ERR_INVALID_INPUT, "%s: the references are not device memory of the handle's GPU %d",
                        is_x ? "set_x_ref_batch_device" : "set_u_ref_batch_device", s->device);
        if ((rc = bind_device(s))) return rc;
        double **store = is_x ? &in.Xi : &in.Ui;
        if (!s->layout_m && !*store && (rc = dalloc(s, store, (size_t)R * C * s->batch))) return rc;
        track = false;  // (the track store stays for the next track; the steps stay)
        *(is_x ? &in.x_const : &in.u_const) = true;  // as when the mode begins: the data of this call decides
    }
    const InstArray a = {src, R, C, is_x ? &in.Xi : &in.Ui, is_x ? s->dXref : s->dUref, is_x ? s->xref_const : s->uref_const,
                         is_x ? &in.x_const : &in.u_const};
    auto shared = is_x ? +[](tinympc_solver *q, const double *const *h) { return tinympc_set_x_ref(q, h[0], q->nx, q->N, 0); }
                       : +[](tinympc_solver *q, const double *const *h) { return tinympc_set_u_ref(q, h[0], q->nu, q->N - 1, 0); };
    return set_inst_batch(s, verb, is_x ? "set_x_ref_batch_device" : "set_u_ref_batch_device", "references", &a, 1, is_x ? in.x : in.u,
                          false, on_device, cols != C, first, count, shared);
}

// tinympc_set_bound_constraints_batch (+ _device): one box (cols = 1) or bounds per knot (cols = N) per instance. Like the shared verb,
// the call enables both bound families.
int set_bounds_batch(tinympc_solver *s, const double *const src[4], bool on_device, int cols, int first, int count) {
    const char *verb = on_device ? "set_bound_constraints_batch_device" : "set_bound_constraints_batch";
    int rc = check_handle(s);
    if (rc) return rc;
    if (!src[0] || !src[1] || !src[2] || !src[3]) return fail(TINYMPC_ERR_INVALID_INPUT, "%s requires x_min, x_max, u_min, u_max", verb);
    const int N = s->N;
    if (cols != N && cols != 1)
        return fail(TINYMPC_ERR_INVALID_INPUT, "%s: cols is %d. Expected %d (bounds per knot) or 1 (one box per instance).", verb, cols, N);
    InstState &in = s->inst;
    const InstArray a[4] = {{src[0], s->nx, N, &in.xmin, s->dxmin, s->xmin_const, &in.bounds_const},
                            {src[1], s->nx, N, &in.xmax, s->dxmax, s->xmax_const, &in.bounds_const},
                            {src[2], s->nu, N - 1, &in.umin, s->dumin, s->umin_const, &in.bounds_const},
                            {src[3], s->nu, N - 1, &in.umax, s->dumax, s->umax_const, &in.bounds_const}};
    auto shared = +[](tinympc_solver *q, const double *const *h) { return tinympc_set_bound_constraints(q, h[0], h[1], h[2], h[3], 0); };
    return set_inst_batch(s, verb, verb, "bounds", a, 4, in.bounds, true, on_device, cols != N, first, count, shared);
}

}  // namespace

int tinympc_set_bound_constraints_batch(tinympc_solver *s, const double *x_min, const double *x_max, const double *u_min,
                                        const double *u_max, int cols, int first, int count) {
    const double *const src[4] = {x_min, x_max, u_min, u_max};
    return set_bounds_batch(s, src, false, cols, first, count);
}
int tinympc_set_bound_constraints_batch_device(tinympc_solver *s, const double *d_x_min, const double *d_x_max, const double *d_u_min,
                                               const double *d_u_max, int cols, int first, int count) {
    const double *const src[4] = {d_x_min, d_x_max, d_u_min, d_u_max};
    return set_bounds_batch(s, src, true, cols, first, count);
}

int tinympc_set_x_ref_batch(tinympc_solver *s, const double *Xrefs, int rows, int cols, int first, int count) {
    return set_ref_batch(s, true, Xrefs, false, rows, cols, first, count);
}
int tinympc_set_u_ref_batch(tinympc_solver *s, const double *Urefs, int rows, int cols, int first, int count) {
    return set_ref_batch(s, false, Urefs, false, rows, cols, first, count);
}
int tinympc_set_x_ref_batch_device(tinympc_solver *s, const double *d_Xrefs, int rows, int cols, int first, int count) {
    return set_ref_batch(s, true, d_Xrefs, true, rows, cols, first, count);
}
int tinympc_set_u_ref_batch_device(tinympc_solver *s, const double *d_Urefs, int rows, int cols, int first, int count) {
    return set_ref_batch(s, false, d_Urefs, true, rows, cols, first, count);
}

namespace {

// hipFree of a block dalloc() made (it leaves the handle's list). Only where nothing queued reads it any more.
void dfree(tinympc_solver *s, void *p) {
    if (!p) return;
    (void)hipStreamSynchronize(s->stream);
    if (!s->session_active) park_sessions_on_device(s->device, s);
    (void)hipFree(p);
    for (size_t i = 0; i < s->allocs.size(); ++i)
        if (s->allocs[i] == p) { s->allocs.erase(s->allocs.begin() + (long)i); break; }
}

// Every instance's step (batched handles): allocated by the first verb that needs it, zeros.
int ensure_ref_steps(tinympc_solver *s) {
    InstState &in = s->inst;
    int rc;
    if (in.steps) return TINYMPC_OK;
    if ((rc = dalloc(s, &in.steps, (size_t)s->batch))) return rc;
    HIP_TRY(hipMemsetAsync(in.steps, 0, sizeof(int) * s->batch, s->stream));
    return TINYMPC_OK;
}

// Single-instance handles: the current window of the host copy of a half's track, through the shared reference verb (pinned-host path,
// session and resident solves included: a window moved up by one knot is what those verbs recognise).
int forward_track_window(tinympc_solver *s, bool is_x) {
    const InstState &in = s->inst;
    const int R = is_x ? s->nx : s->nu, C = is_x ? s->N : s->N - 1, T = is_x ? in.Tx : in.Tu;
    const std::vector<double> &track = is_x ? in.hXt : in.hUt;
    std::vector<double> w((size_t)R * C);
    for (int k = 0; k < C; ++k) {
        const long col = (long)in.hstep + k < T ? (long)in.hstep + k : T - 1;
        std::memcpy(w.data() + (size_t)k * R, track.data() + (size_t)col * R, sizeof(double) * R);
    }
    return is_x ? set_x_ref_shared(s, w.data(), R, C, 0, true) : set_u_ref_shared(s, w.data(), R, C, 0, true);
}
int forward_track_windows(tinympc_solver *s) {
    int rc;
    if (s->inst.x_track && (rc = forward_track_window(s, true))) return rc;
    if (s->inst.u_track && (rc = forward_track_window(s, false))) return rc;
    return TINYMPC_OK;
}

// tinympc_set_x_ref_track_batch / _u_ref_track_batch (+ _device): T knots of one half of the references per instance, kept on the
// device; the rows of the window the instance's step selects are built there (k_build_inst_tables). Everything is validated, and every
// block the call needs allocated, before anything is written; the upload itself is the per-instance verbs' (set_inst_batch, cols = T).
int set_ref_track(tinympc_solver *s, bool is_x, const double *src, bool on_device, int rows, int T, int first, int count) {
    const char *verb = is_x ? (on_device ? "set_x_ref_track_batch_device" : "set_x_ref_track_batch")
                            : (on_device ? "set_u_ref_track_batch_device" : "set_u_ref_track_batch");
    int rc = check_handle(s);
    if (rc) return rc;
    if (!src) return fail(TINYMPC_ERR_INVALID_INPUT, "%s: the tracks are NULL", verb);
    const int R = is_x ? s->nx : s->nu;
    if (rows != R || T < 1)
        return fail(TINYMPC_ERR_INVALID_INPUT, "%s: the tracks are %d x %d per instance. Expected %d x T with T >= 1.", verb, rows, T, R);
    if (first < 0 || count < 0 || first + count > s->batch)
        return fail(TINYMPC_ERR_INVALID_INPUT, "%s: instance range [%d, %d) outside batch of %d", verb, first, first + count, s->batch);
    if (on_device && count > 0 && !on_handles_device(s, src))
        return fail(TINYMPC_ERR_INVALID_INPUT, "%s: the tracks are not device memory of the handle's GPU %d", verb, s->device);
    InstState &in = s->inst;
    bool &track = is_x ? in.x_track : in.u_track, &mode = is_x ? in.x : in.u;
    int &Tcur = is_x ? in.Tx : in.Tu;
    const bool whole = first == 0 && count == s->batch;
    if (!track && !whole)
        return fail(TINYMPC_ERR_INVALID_INPUT, "%s: the first track call of a half must name the whole batch (first = 0, count = %d)", verb, s->batch);
    if (track && !whole && T != Tcur)
        return fail(TINYMPC_ERR_INVALID_INPUT, "%s: a call on a sub-range must keep the track length T = %d (got %d); a whole-batch call may change it",
                    verb, Tcur, T);
    const size_t per = (size_t)R * T;
    if (s->batch == 1) {  // the host copy; the current window goes through the shared verb
        if (count == 0) return TINYMPC_OK;
        std::vector<double> h(per);
        if (on_device) {
            if ((rc = bind_device(s))) return rc;
            if ((rc = download(s, h.data(), src, sizeof(double) * per))) return rc;
        } else {
            std::memcpy(h.data(), src, sizeof(double) * per);
        }
        (is_x ? in.hXt : in.hUt).swap(h);
        Tcur = T;
        track = true;
        return forward_track_window(s, is_x);
    }
    if ((rc = bind_device(s))) return rc;
    double *&store = is_x ? in.Xt : in.Ut;
    size_t &cap = is_x ? in.xt_cap : in.ut_cap;
    double *grown = nullptr;
    if (!s->layout_m) {  // (layout M: no kernel carries per-instance references -- the next launch refuses, as for trajectories)
        if ((rc = ensure_ref_steps(s)) || (rc = alloc_inst_rows(s, in.models))) return rc;
        if (per * s->batch > cap && (rc = dalloc(s, &grown, per * s->batch))) return rc;
    }
    // the upload, into the new store where the call needed one; mode, store and T change only after it has succeeded
    double *dst = grown ? grown : store;
    bool on = true;  // (set_inst_batch: the mode counts as on -- nothing is filled from the shared reference, the whole batch has been named)
    const InstArray a = {src, R, T, &dst, nullptr, false, nullptr};
    if ((rc = set_inst_batch(s, verb, verb, "tracks", &a, 1, on, false, on_device, false, first, count, nullptr))) {
        dfree(s, grown);
        return rc;
    }
    if (grown) {  // (a whole-batch call: nothing of the old store is kept)
        dfree(s, store);
        store = grown;
        cap = per * s->batch;
    }
    Tcur = T;
    track = true;
    mode = true;
    *(is_x ? &in.x_const : &in.u_const) = false;  // (even T = 1: a track is a trajectory, layout A)
    return TINYMPC_OK;
}

// tinympc_set_ref_step_batch (+ _device).
int set_ref_steps(tinympc_solver *s, const int *steps, bool on_device, int first, int count) {
    const char *verb = on_device ? "set_ref_step_batch_device" : "set_ref_step_batch";
    int rc = check_handle(s);
    if (rc) return rc;
    if (!steps) return fail(TINYMPC_ERR_INVALID_INPUT, "%s: steps is NULL", verb);
    if (first < 0 || count < 0 || first + count > s->batch)
        return fail(TINYMPC_ERR_INVALID_INPUT, "%s: instance range [%d, %d) outside batch of %d", verb, first, first + count, s->batch);
    InstState &in = s->inst;
    if (count == 0) return TINYMPC_OK;
    if (on_device) {
        if (!on_handles_device(s, steps))
            return fail(TINYMPC_ERR_INVALID_INPUT, "%s: the steps are not device memory of the handle's GPU %d", verb, s->device);
        if ((rc = bind_device(s))) return rc;
        if (!in.mflag && (rc = dalloc(s, &in.mflag, (size_t)1))) return rc;
        int bad = 0;
        HIP_TRY(hipMemsetAsync(in.mflag, 0, sizeof(int), s->stream));
        HIP_TRY(launch_check_ref_steps(steps, count, 0, in.mflag, s->stream));
        if ((rc = download(s, &bad, in.mflag, sizeof(int)))) return rc;
        if (bad) return fail(TINYMPC_ERR_INVALID_INPUT, "%s: every step must be >= 0", verb);
    } else {
        for (int b = 0; b < count; ++b)
            if (steps[b] < 0) return fail(TINYMPC_ERR_INVALID_INPUT, "%s: steps[%d] = %d. Expected a step >= 0.", verb, b, steps[b]);
    }
    if (s->batch == 1) {
        int v = 0;
        if (on_device) { if ((rc = download(s, &v, steps, sizeof(int)))) return rc; }
        else v = steps[0];
        in.hstep = v;
        return forward_track_windows(s);
    }
    if (!on_device && (rc = bind_device(s))) return rc;
    if ((rc = ensure_ref_steps(s))) return rc;
    HIP_TRY(hipMemcpyAsync(in.steps + first, steps, sizeof(int) * count, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));  // (the caller keeps ownership of its buffer: copied when the call returns)
    if (in.tracks()) in.mark(first, first + count);
    return TINYMPC_OK;
}

// Every instance's step += delta (delta >= 0 here, or validated by the caller), on the handle's stream: no copy, no synchronisation. The
// rows are rebuilt at the next launch (refresh_inst_tables).
int advance_ref_steps(tinympc_solver *s, int delta) {
    InstState &in = s->inst;
    if (s->batch == 1) {
        const long v = (long)in.hstep + delta;
        in.hstep = v < 0 ? 0 : v > 2147483647L ? 2147483647 : (int)v;
        return forward_track_windows(s);
    }
    int rc;
    if ((rc = ensure_ref_steps(s))) return rc;
    HIP_TRY(launch_advance_ref_steps(in.steps, s->batch, delta, s->stream));
    if (in.tracks()) in.mark(0, s->batch);
    return TINYMPC_OK;
}

}  // namespace

static int advance_ref_steps_after_tick(tinympc_solver *s) { return advance_ref_steps(s, s->inst.auto_advance); }

int tinympc_set_x_ref_track_batch(tinympc_solver *s, const double *Xtracks, int rows, int T, int first, int count) {
    return set_ref_track(s, true, Xtracks, false, rows, T, first, count);
}
int tinympc_set_u_ref_track_batch(tinympc_solver *s, const double *Utracks, int rows, int T, int first, int count) {
    return set_ref_track(s, false, Utracks, false, rows, T, first, count);
}
int tinympc_set_x_ref_track_batch_device(tinympc_solver *s, const double *d_Xtracks, int rows, int T, int first, int count) {
    return set_ref_track(s, true, d_Xtracks, true, rows, T, first, count);
}
int tinympc_set_u_ref_track_batch_device(tinympc_solver *s, const double *d_Utracks, int rows, int T, int first, int count) {
    return set_ref_track(s, false, d_Utracks, true, rows, T, first, count);
}
int tinympc_set_ref_step_batch(tinympc_solver *s, const int *steps, int first, int count) { return set_ref_steps(s, steps, false, first, count); }
int tinympc_set_ref_step_batch_device(tinympc_solver *s, const int *d_steps, int first, int count) { return set_ref_steps(s, d_steps, true, first, count); }

int tinympc_advance_ref_step_batch(tinympc_solver *s, int delta) {
    int rc = check_handle(s);
    if (rc) return rc;
    InstState &in = s->inst;
    if (s->batch == 1) {
        if ((long)in.hstep + delta < 0)
            return fail(TINYMPC_ERR_INVALID_INPUT, "advance_ref_step_batch: step %d + delta %d is negative", in.hstep, delta);
        return advance_ref_steps(s, delta);
    }
    if ((rc = bind_device(s))) return rc;
    if (delta < 0) {  // going back: validated on the device first (one flag read back; an advance by delta >= 0 reads nothing back)
        if (!in.steps) return fail(TINYMPC_ERR_INVALID_INPUT, "advance_ref_step_batch: delta %d would take a step below 0", delta);
        if (!in.mflag && (rc = dalloc(s, &in.mflag, (size_t)1))) return rc;
        int bad = 0;
        HIP_TRY(hipMemsetAsync(in.mflag, 0, sizeof(int), s->stream));
        HIP_TRY(launch_check_ref_steps(in.steps, s->batch, delta, in.mflag, s->stream));
        if ((rc = download(s, &bad, in.mflag, sizeof(int)))) return rc;
        if (bad) return fail(TINYMPC_ERR_INVALID_INPUT, "advance_ref_step_batch: delta %d would take a step below 0", delta);
    }
    return advance_ref_steps(s, delta);
}

int tinympc_set_ref_auto_advance(tinympc_solver *s, int delta) {
    int rc = check_handle(s);
    if (rc) return rc;
    // (the tick reads nothing back, so it cannot validate: only advances that need no validation)
    if (delta < 0) return fail(TINYMPC_ERR_INVALID_INPUT, "set_ref_auto_advance: delta must be >= 0 (got %d)", delta);
    if (delta > 0 && s->batch > 1) {  // (the step array now, not inside the first tick)
        if ((rc = bind_device(s))) return rc;
        if ((rc = ensure_ref_steps(s))) return rc;
    }
    s->inst.auto_advance = delta;
    return TINYMPC_OK;
}

int tinympc_get_ref_step_batch(tinympc_solver *s, int *steps_out, int first, int count) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (!steps_out || first < 0 || count < 0 || first + count > s->batch)
        return fail(TINYMPC_ERR_INVALID_INPUT, "get_ref_step_batch: range [%d, %d) outside the batch of %d", first, first + count, s->batch);
    if (count == 0) return TINYMPC_OK;
    if (s->batch == 1) { steps_out[0] = s->inst.hstep; return TINYMPC_OK; }
    if (!s->inst.steps) { std::memset(steps_out, 0, sizeof(int) * count); return TINYMPC_OK; }  // (steps start at 0)
    if ((rc = bind_device(s))) return rc;
    return download(s, steps_out, s->inst.steps + first, sizeof(int) * count);
}

namespace {

// Batched precompute + operator builder for instances [first, first+count) of the per-instance model store (InstState): one wavefront
// (k_precompute_rows) or workgroup (k_precompute) per instance -- the kernels, and so the caches, of a single-instance setup.
int precompute_inst_models(tinympc_solver *s, int first, int count) {
    InstState &in = s->inst;
    const size_t nx = s->nx, nu = s->nu;
    const char *env = getenv("TINYMPC_PRECOMPUTE");
    const bool rows = precompute_rows_supported(s->nx, s->nu) && !(env && (env[0] == 'l' || env[0] == 'L'));
    const size_t ws = precompute_scratch_doubles(s->nx, s->nu) + 8;
    const bool use_lds = precompute_scratch_doubles(s->nx, s->nu) <= 6500;
    // (working sets beyond LDS live in global scratch: at most kChunk instances per launch share one block of it)
    constexpr int kChunk = 256;
    const int chunk = (rows || use_lds) ? count : kChunk;
    int rc;
    if (!rows && !use_lds && !in.mscratch && (rc = dalloc(s, &in.mscratch, ws * kChunk))) return rc;
    for (int b0 = first; b0 < first + count; b0 += chunk) {
        const int n = first + count - b0 < chunk ? first + count - b0 : chunk;
        PrecomputeParams p{};
        p.nx = s->nx; p.nu = s->nu; p.rho_sys = in.mrho + b0;  // (indexed by the launch's blockIdx.x: the ABSOLUTE instance b0 + b)
        p.A = in.mA + b0 * nx * nx; p.B = in.mB + b0 * nx * nu; p.fdyn = in.mf + b0 * nx; p.Qd = in.mQd + b0 * nx; p.Rd = in.mRd + b0 * nu;
        p.Kinf = in.cK + b0 * nu * nx; p.Pinf = in.cP + b0 * nx * nx; p.Quu_inv = in.cQuu + b0 * nu * nu; p.AmBKt = in.cAm + b0 * nx * nx;
        p.APf = in.cAPf + b0 * nx; p.BPf = in.cBPf + b0 * nu;
        p.info = in.cinfo + (size_t)b0 * 4; p.scratch = in.mscratch; p.scratch_stride = ws;
        p.use_lds = use_lds ? 1 : 0;
        p.count = n;
        if (rows) HIP_TRY(launch_precompute_rows(p, s->stream));
        else HIP_TRY(launch_precompute(p, s->stream));
    }
    OperatorParams o{};
    o.nx = s->nx; o.nu = s->nu; o.W = s->W; o.KT = s->KT;
    o.A = in.mA + first * nx * nx; o.B = in.mB + first * nx * nu; o.fdyn = in.mf + first * nx; o.Qd = in.mQd + first * nx; o.Rd = in.mRd + first * nu;
    o.Kinf = in.cK + first * nu * nx; o.Quu_inv = in.cQuu + first * nu * nu; o.AmBKt = in.cAm + first * nx * nx;
    o.APf = in.cAPf + first * nx; o.BPf = in.cBPf + first * nu;
    o.ops = in.ops + (size_t)first * ops_doubles(s->W, s->KT);
    o.count = count;
    HIP_TRY(launch_build_operators(o, s->stream));
    return TINYMPC_OK;
}

// The per-instance model mode begins (the first tinympc_set_model_batch or tinympc_set_rho_batch): the stores, and every instance <- the
// shared model, cache, operators and rho of this moment.
int enter_model_mode(tinympc_solver *s) {
    InstState &in = s->inst;
    int rc;
    if (!in.mrho && (rc = dalloc(s, &in.mrho, (size_t)s->batch))) return rc;
    if (s->layout_m) {  // (no kernel carries the mode: the next launch refuses until tinympc_clear_model_batch)
        if (!in.models) HIP_TRY(launch_fill(in.mrho, (size_t)s->batch, s->rho, s->stream));
        in.models = true;
        return TINYMPC_OK;
    }
    const size_t nx = s->nx, nu = s->nu, batch = s->batch, od = ops_doubles(s->W, s->KT);
    if (!in.ops) {
        if ((rc = dalloc(s, &in.mA, nx * nx * batch)) || (rc = dalloc(s, &in.mB, nx * nu * batch)) || (rc = dalloc(s, &in.mf, nx * batch)) ||
            (rc = dalloc(s, &in.mQd, nx * batch)) || (rc = dalloc(s, &in.mRd, nu * batch)) || (rc = dalloc(s, &in.cK, nu * nx * batch)) ||
            (rc = dalloc(s, &in.cP, nx * nx * batch)) || (rc = dalloc(s, &in.cQuu, nu * nu * batch)) || (rc = dalloc(s, &in.cAm, nx * nx * batch)) ||
            (rc = dalloc(s, &in.cAPf, nx * batch)) || (rc = dalloc(s, &in.cBPf, nu * batch)) || (rc = dalloc(s, &in.cinfo, 4 * batch)) ||
            (rc = dalloc(s, &in.mstage, (nx + nu) * batch)) || (rc = dalloc(s, &in.mQ0, nx * batch)) || (rc = dalloc(s, &in.mR0, nu * batch)) ||
            (rc = dalloc(s, &in.ops, od * batch)))
            return rc;
        HIP_TRY(hipMemsetAsync(in.cinfo, 0, sizeof(int) * 4 * batch, s->stream));
    }
    if ((rc = alloc_inst_rows(s, true))) return rc;
    if (!in.models) {  // every instance starts from the shared model of this moment
        // (references a single-instance handle holds in pinned host memory: the per-instance rows are built from the device copies)
        if (s->refs_on_host && (rc = flush_host_refs(s))) return rc;
        if ((rc = refresh_derived(s))) return rc;  // (the shared operator block, from the shared cache as it is now)
        InstModelFillParams f{};
        f.batch = s->batch;
        const struct { const double *src; double *dst; size_t n; } seg[] = {
            {s->dA, in.mA, nx * nx}, {s->dB, in.mB, nx * nu}, {s->dfdyn, in.mf, nx}, {s->dQd, in.mQd, nx}, {s->dRd, in.mRd, nu},
            {s->dKinf, in.cK, nu * nx}, {s->dPinf, in.cP, nx * nx}, {s->dQuu, in.cQuu, nu * nu}, {s->dAmBKt, in.cAm, nx * nx},
            {s->dAPf, in.cAPf, nx}, {s->dBPf, in.cBPf, nu}, {s->dops, in.ops, od}};
        f.nseg = 12;
        for (int i = 0; i < 12; ++i) { f.seg[i].src = seg[i].src; f.seg[i].dst = seg[i].dst; f.seg[i].n = (int)seg[i].n; }
        f.info_src = s->dinfo; f.info_dst = in.cinfo;
        HIP_TRY(launch_fill_inst_models(f, s->stream));
        // ... the raw diagonals of the shared Q and R (setup's device copies of the full matrices), and the shared rho
        InstDiagParams q0{}, r0{};
        q0.src = s->dQfull; q0.src_step = s->nx + 1; q0.n = s->nx; q0.dst = in.mQ0;
        r0.src = s->dRfull; r0.src_step = s->nu + 1; r0.n = s->nu; r0.dst = in.mR0;
        q0.count = r0.count = s->batch;  // (src_stride 0: the one shared matrix for every instance)
        HIP_TRY(launch_store_inst_diag(q0, s->stream));
        HIP_TRY(launch_store_inst_diag(r0, s->stream));
        HIP_TRY(launch_fill(in.mrho, batch, s->rho, s->stream));
        in.models = true;
        in.mark(0, s->batch);
    }
    return TINYMPC_OK;
}

// Qd_b = Q0_b + rho_b, Rd_b = R0_b + rho_b for instances [first, first+count): ONE addition from the raw diagonals, as tinympc_setup forms
// them (tiny_api.cpp:90-91), then the instances' caches and operators (precompute_inst_models); their table rows are rebuilt at the next
// launch (refresh_inst_tables). What both per-instance model verbs end with.
int rebuild_inst_models(tinympc_solver *s, int first, int count) {
    InstState &in = s->inst;
    InstDiagParams dq{}, dr{};
    dq.n = s->nx; dr.n = s->nu;
    dq.first = dr.first = first; dq.count = dr.count = count; dq.add_inst = dr.add_inst = in.mrho;
    dq.src = in.mQ0 + (size_t)first * s->nx; dq.src_stride = s->nx; dq.src_step = 1; dq.dst = in.mQd;
    dr.src = in.mR0 + (size_t)first * s->nu; dr.src_stride = s->nu; dr.src_step = 1; dr.dst = in.mRd;
    HIP_TRY(launch_store_inst_diag(dq, s->stream));
    HIP_TRY(launch_store_inst_diag(dr, s->stream));
    int rc;
    if ((rc = precompute_inst_models(s, first, count))) return rc;
    in.mark(first, first + count);
    return TINYMPC_OK;
}

// tinympc_set_model_batch (+ _device). The mode enters at the first call: every instance then holds the shared model, cache and
// operators of that moment; the instances named here get their own (precompute_inst_models), and their table rows are rebuilt at the
// next launch from their own Pinf and cost diagonals (refresh_inst_tables).
int set_model_batch(tinympc_solver *s, const double *A, const double *B, const double *fdyn, const double *Q, const double *R, bool on_device,
                    int first, int count) {
    const char *verb = on_device ? "set_model_batch_device" : "set_model_batch";
    int rc = check_handle(s);
    if (rc) return rc;
    if (!A || !B || !Q || !R) return fail(TINYMPC_ERR_INVALID_INPUT, "%s requires A, B, Q, R", verb);
    if (first < 0 || count < 1 || first + count > s->batch)
        return fail(TINYMPC_ERR_INVALID_INPUT, "%s: instance range [%d, %d) is empty or outside batch of %d", verb, first, first + count, s->batch);
    const double *src[5] = {A, B, fdyn, Q, R};
    for (int i = 0; on_device && i < 5; ++i)  // device memory of the handle's own GPU (a host pointer or another GPU's memory is refused here)
        if (src[i] && !on_handles_device(s, src[i]))
            return fail(TINYMPC_ERR_INVALID_INPUT, "%s: the models are not device memory of the handle's GPU %d", verb, s->device);
    if ((rc = bind_device(s))) return rc;
    InstState &in = s->inst;
    if ((rc = enter_model_mode(s))) return rc;
    if (s->layout_m) return TINYMPC_OK;
    const size_t nx = s->nx, nu = s->nu;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    HIP_TRY(hipMemcpyAsync(in.mA + first * nx * nx, A, sizeof(double) * nx * nx * count, kind, s->stream));
    HIP_TRY(hipMemcpyAsync(in.mB + first * nx * nu, B, sizeof(double) * nx * nu * count, kind, s->stream));
    if (fdyn) HIP_TRY(hipMemcpyAsync(in.mf + first * nx, fdyn, sizeof(double) * nx * count, kind, s->stream));
    else HIP_TRY(hipMemsetAsync(in.mf + first * nx, 0, sizeof(double) * nx * count, s->stream));
    // the raw cost diagonals: from the caller's device memory as it lies, from host memory gathered first (rebuild_inst_models adds rho)
    std::vector<double> hd;
    InstDiagParams dq{}, dr{};
    dq.n = s->nx; dr.n = s->nu;
    dq.first = dr.first = first; dq.count = dr.count = count;
    dq.dst = in.mQ0; dr.dst = in.mR0;
    if (on_device) {
        dq.src = Q; dq.src_stride = nx * nx; dq.src_step = s->nx + 1;
        dr.src = R; dr.src_stride = nu * nu; dr.src_step = s->nu + 1;
    } else {
        hd.resize((nx + nu) * count);
        for (size_t b = 0; b < (size_t)count; ++b) {
            for (size_t i = 0; i < nx; ++i) hd[b * nx + i] = Q[b * nx * nx + i * (nx + 1)];
            for (size_t i = 0; i < nu; ++i) hd[nx * count + b * nu + i] = R[b * nu * nu + i * (nu + 1)];
        }
        HIP_TRY(hipMemcpyAsync(in.mstage, hd.data(), sizeof(double) * hd.size(), hipMemcpyHostToDevice, s->stream));
        dq.src = in.mstage; dq.src_stride = nx; dq.src_step = 1;
        dr.src = in.mstage + nx * count; dr.src_stride = nu; dr.src_step = 1;
    }
    HIP_TRY(launch_store_inst_diag(dq, s->stream));
    HIP_TRY(launch_store_inst_diag(dr, s->stream));
    if ((rc = rebuild_inst_models(s, first, count))) return rc;
    // the caller keeps ownership of its buffers: the copies have completed when the call returns (the tinympc_set_x0_batch_device rule)
    HIP_TRY(hipStreamSynchronize(s->stream));
    return TINYMPC_OK;
}

// tinympc_set_rho_batch (+ _device): the same mode, entered the same way; the instances named here get their own rho, and with it their
// own Qd + rho, cache, operators and table rows -- from the raw diagonals of whatever model they hold, so the order of the two verbs
// does not matter. Everything is validated before anything is written (device input: on the device, one flag read back).
int set_rho_batch(tinympc_solver *s, const double *rho, bool on_device, int first, int count) {
    const char *verb = on_device ? "set_rho_batch_device" : "set_rho_batch";
    int rc = check_handle(s);
    if (rc) return rc;
    if (!rho) return fail(TINYMPC_ERR_INVALID_INPUT, "%s requires rho", verb);
    if (first < 0 || count < 1 || first + count > s->batch)
        return fail(TINYMPC_ERR_INVALID_INPUT, "%s: instance range [%d, %d) is empty or outside batch of %d", verb, first, first + count, s->batch);
    InstState &in = s->inst;
    if (on_device) {
        if (!on_handles_device(s, rho))
            return fail(TINYMPC_ERR_INVALID_INPUT, "%s: rho is not device memory of the handle's GPU %d", verb, s->device);
        if ((rc = bind_device(s))) return rc;
        if (!in.mflag && (rc = dalloc(s, &in.mflag, (size_t)1))) return rc;
        int bad = 0;
        HIP_TRY(hipMemsetAsync(in.mflag, 0, sizeof(int), s->stream));
        HIP_TRY(launch_check_positive(rho, count, in.mflag, s->stream));
        if ((rc = download(s, &bad, in.mflag, sizeof(int)))) return rc;
        if (bad) return fail(TINYMPC_ERR_INVALID_INPUT, "%s: every rho must be a finite number > 0", verb);
    } else {
        for (int b = 0; b < count; ++b)
            if (!(rho[b] > 0.0) || !std::isfinite(rho[b]))
                return fail(TINYMPC_ERR_INVALID_INPUT, "%s: rho[%d] = %g. Expected a finite number > 0.", verb, b, rho[b]);
        if ((rc = bind_device(s))) return rc;
    }
    if ((rc = enter_model_mode(s))) return rc;
    in.rho_verb = true;
    HIP_TRY(hipMemcpyAsync(in.mrho + first, rho, sizeof(double) * count, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s->stream));
    if (!s->layout_m && (rc = rebuild_inst_models(s, first, count))) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));  // (the caller keeps ownership of its buffer: copied when the call returns)
    return TINYMPC_OK;
}

// tinympc_set_linear_constraints_batch (+ _device): the linear rows of instances [first, first+count). Host input is staged on the device;
// from there both forms are ONE path -- k_check_inst_lin validates the arrays where they lie (one flag read back), then, and only
// then, k_build_inst_lin writes the instances' rows into the store the kernel reads. Nothing else is kept.
// tinympc_set_linear_constraints_knots_batch (+ _device) is the same path with per_knot set: the arrays hold the rows of every knot (N
// blocks per instance on the state side, N-1 on the input side), k_check_inst_lin walks them as (instance, knot) pairs and
// k_build_inst_lin_knots writes the store's knot slots.
int set_lin_batch(tinympc_solver *s, const double *Ax, const double *bx, int nlx, const double *Au, const double *bu, int nlu, bool on_device,
                  int first, int count, bool per_knot = false) {
    const char *verb = per_knot ? (on_device ? "set_linear_constraints_knots_batch_device" : "set_linear_constraints_knots_batch")
                                : (on_device ? "set_linear_constraints_batch_device" : "set_linear_constraints_batch");
    int rc = check_handle(s);
    if (rc) return rc;
    if (nlx < 0 || nlu < 0) return fail(TINYMPC_ERR_INVALID_INPUT, "%s: negative constraint count", verb);
    if ((nlx > 0 && (!Ax || !bx)) || (nlu > 0 && (!Au || !bu)))
        return fail(TINYMPC_ERR_INVALID_INPUT, "%s: NULL array for a non-empty side", verb);
    if (nlx + nlu == 0)
        return fail(TINYMPC_ERR_INVALID_INPUT, "%s: no rows on either side (tinympc_set_linear_constraints with no rows clears the family)", verb);
    if (first < 0 || count < 1 || first + count > s->batch)
        return fail(TINYMPC_ERR_INVALID_INPUT, "%s: instance range [%d, %d) is empty or outside batch of %d", verb, first, first + count, s->batch);
    if (nlx > MAX_LIN_ROWS || nlu > MAX_LIN_ROWS)
        return fail(TINYMPC_ERR_UNSUPPORTED, "%s: at most %d rows per side (got %d state, %d input): per-instance rows run on the generic kernel only",
                    verb, MAX_LIN_ROWS, nlx, nlu);
    if (per_knot && s->batch == 1)
        return fail(TINYMPC_ERR_UNSUPPORTED, "%s: single-instance handles run on the shared description: per-knot rows need a batched handle", verb);
    const size_t nx = s->nx, nu = s->nu, ax = (size_t)nlx * nx, au = (size_t)nlu * nu, n = (size_t)count;
    const size_t kx = per_knot ? (size_t)s->N : 1, ku = per_knot ? (size_t)s->N - 1 : 1;  // blocks of rows per instance and side
    if (on_device && ((nlx > 0 && (!on_handles_device(s, Ax) || !on_handles_device(s, bx))) || (nlu > 0 && (!on_handles_device(s, Au) || !on_handles_device(s, bu)))))
        return fail(TINYMPC_ERR_INVALID_INPUT, "%s: the rows are not device memory of the handle's GPU %d", verb, s->device);
    InstState &in = s->inst;
    if (s->batch == 1) {  // the shared verb, after this verb's own checks of the values
        std::vector<double> h(ax + nlx + au + nlu);
        double *hAx = h.data(), *hbx = hAx + ax, *hAu = hbx + nlx, *hbu = hAu + au;
        const double *src[4] = {Ax, bx, Au, bu};
        double *dst[4] = {hAx, hbx, hAu, hbu};
        const size_t len[4] = {ax, (size_t)nlx, au, (size_t)nlu};
        if (on_device && (rc = bind_device(s))) return rc;
        for (int i = 0; i < 4; ++i) {
            if (!len[i]) continue;
            if (on_device) { if ((rc = download(s, dst[i], src[i], sizeof(double) * len[i]))) return rc; }
            else std::memcpy(dst[i], src[i], sizeof(double) * len[i]);
        }
        for (size_t i = 0; i < ax + nlx + au + nlu; ++i) {
            const bool is_b = (i >= ax && i < ax + nlx) || i >= ax + nlx + au;
            if (is_b ? !(h[i] >= -1.79769313486231570815e308) : !std::isfinite(h[i]))
                return fail(TINYMPC_ERR_INVALID_INPUT, "%s: a row of A must be finite and not all zero, b a number or +inf", verb);
        }
        return tinympc_set_linear_constraints(s, hAx, hbx, nlx, hAu, hbu, nlu);
    }
    // the counts belong to the batch: a sub-range keeps them -- the mode's, or those of the shared rows the other instances stay on
    const bool whole = first == 0 && count == s->batch;
    const bool same = in.lin ? (nlx == in.lin_nlx && nlu == in.lin_nlu)
                             : (nlx == s->n_lin_x && nlu == s->n_lin_u && s->Alin_x.size() == ax && s->Alin_u.size() == au);
    // the per-knot form: a sub-range only replaces rows of a store that is already per knot; and only a whole batch leaves it
    if (per_knot && !whole && !in.lin_knots)
        return fail(TINYMPC_ERR_INVALID_INPUT, "%s: the first call must name the whole batch (first = 0, count = %d), got instances [%d, %d)", verb,
                    s->batch, first, first + count);
    if (!per_knot && !whole && in.lin_knots)
        return fail(TINYMPC_ERR_INVALID_INPUT, "%s: the handle's rows are per knot (set_linear_constraints_knots_batch): name the whole batch "
                    "(first = 0, count = %d) to return to rows constant over the horizon", verb, s->batch);
    if (!whole && !same)
        return fail(TINYMPC_ERR_INVALID_INPUT, "%s: %d state and %d input rows for instances [%d, %d) of %d, but %s %d and %d: name the whole batch "
                    "(first = 0, count = %d) to %s", verb, nlx, nlu, first, first + count, s->batch,
                    in.lin ? "the mode's counts are" : "the handle's shared rows are", in.lin ? in.lin_nlx : s->n_lin_x, in.lin ? in.lin_nlu : s->n_lin_u,
                    s->batch, in.lin ? "change the counts" : "begin the mode with counts of its own");
    if ((rc = bind_device(s))) return rc;
    InstLinParams q{};
    q.nx = s->nx; q.nu = s->nu; q.W = s->W; q.nlx = nlx; q.nlu = nlu; q.nl = nlx > nlu ? nlx : nlu;
    q.batch = s->batch; q.first = first; q.count = count;
    q.ax_stride = ax * kx; q.bx_stride = (size_t)nlx * kx; q.au_stride = au * ku; q.bu_stride = (size_t)nlu * ku;
    if (per_knot) { q.knots = s->N; q.ax_knot = ax; q.bx_knot = (size_t)nlx; q.au_knot = au; q.bu_knot = (size_t)nlu; }
    const size_t per = (ax + nlx) * kx + (au + nlu) * ku;
    double *old_stage = nullptr, *old_rows = nullptr;
    if (on_device) {
        q.Ax = Ax; q.bx = bx; q.Au = Au; q.bu = bu;
    } else {
        if (per * n > in.lstage_cap) {
            old_stage = in.lstage;
            if ((rc = dalloc(s, &in.lstage, per * n))) return rc;
            in.lstage_cap = per * n;
        }
        double *dAx = in.lstage, *dbx = dAx + ax * kx * n, *dAu = dbx + nlx * kx * n, *dbu = dAu + au * ku * n;
        if (nlx > 0) {
            HIP_TRY(hipMemcpyAsync(dAx, Ax, sizeof(double) * ax * kx * n, hipMemcpyHostToDevice, s->stream));
            HIP_TRY(hipMemcpyAsync(dbx, bx, sizeof(double) * nlx * kx * n, hipMemcpyHostToDevice, s->stream));
        }
        if (nlu > 0) {
            HIP_TRY(hipMemcpyAsync(dAu, Au, sizeof(double) * au * ku * n, hipMemcpyHostToDevice, s->stream));
            HIP_TRY(hipMemcpyAsync(dbu, bu, sizeof(double) * nlu * ku * n, hipMemcpyHostToDevice, s->stream));
        }
        q.Ax = dAx; q.bx = dbx; q.Au = dAu; q.bu = dbu;
    }
    if (!in.mflag && (rc = dalloc(s, &in.mflag, (size_t)1))) return rc;
    int bad = 0;
    HIP_TRY(hipMemsetAsync(in.mflag, 0, sizeof(int), s->stream));
    if (per_knot) {  // the rows of every (instance, knot) pair, a side at a time (the sides differ in their knots): blocks ax / au apart
        InstLinParams c = q;
        c.nlu = 0; c.count = count * (int)kx; c.ax_stride = ax; c.bx_stride = (size_t)nlx;
        HIP_TRY(launch_check_inst_lin(c, in.mflag, s->stream));
        c = q;
        c.nlx = 0; c.count = count * (int)ku; c.au_stride = au; c.bu_stride = (size_t)nlu;
        HIP_TRY(launch_check_inst_lin(c, in.mflag, s->stream));
    } else HIP_TRY(launch_check_inst_lin(q, in.mflag, s->stream));
    if ((rc = download(s, &bad, in.mflag, sizeof(int)))) return rc;  // (host input has been copied when this returns)
    if (old_stage) dfree(s, old_stage);
    if (bad)
        return fail(TINYMPC_ERR_INVALID_INPUT, "%s: a row of A is all zero or not finite, or a b is NaN or -inf (b = +inf switches a row off)", verb);
    // ---- valid: from here on the call writes
    if (!s->layout_m) {  // (large systems: no kernel carries the mode -- the next solve refuses until the shared verb clears it)
        if ((rc = alloc_inst_rows(s, true))) return rc;
        const size_t need = inst_lin_store_doubles(s->groups, q.nl, q.knots);
        if (need > in.lrows_cap) {
            old_rows = in.lrows;
            if ((rc = dalloc(s, &in.lrows, need))) return rc;
            in.lrows_cap = need;
        }
        q.dst = in.lrows;
        // the store begins (or changes its row count, or moves between rows per knot and rows constant over the horizon): every lane absent,
        // padding included ...
        if (!in.lin || q.nl != in.lin_nl || q.knots != in.lin_knots || old_rows) {
            InstLinParams z = q;
            z.nlx = z.nlu = 0; z.first = 0; z.count = s->groups * s->IPW;
            z.Ax = z.bx = z.Au = z.bu = nullptr;
            HIP_TRY(per_knot ? launch_build_inst_lin_knots(z, s->stream) : launch_build_inst_lin(z, s->stream));
            in.slopes_dirty = true;  // (the groups' slope vectors share the blocks that were just laid out anew: rebuilt at the next launch)
            if (!whole) {  // ... and the instances this call does not name on the shared rows of this moment (same counts: checked above)
                double *sh = nullptr;
                if ((rc = dalloc(s, &sh, per))) return rc;
                std::vector<double> h;
                h.insert(h.end(), s->Alin_x.begin(), s->Alin_x.end()); h.insert(h.end(), s->blin_x.begin(), s->blin_x.end());
                h.insert(h.end(), s->Alin_u.begin(), s->Alin_u.end()); h.insert(h.end(), s->blin_u.begin(), s->blin_u.end());
                HIP_TRY(hipMemcpyAsync(sh, h.data(), sizeof(double) * per, hipMemcpyHostToDevice, s->stream));
                InstLinParams w = q;
                w.first = 0; w.count = s->batch;
                w.Ax = sh; w.bx = sh + ax; w.Au = w.bx + nlx; w.bu = w.Au + au;
                w.ax_stride = w.bx_stride = w.au_stride = w.bu_stride = 0;
                HIP_TRY(launch_build_inst_lin(w, s->stream));
                HIP_TRY(hipStreamSynchronize(s->stream));  // (h and sh end here)
                dfree(s, sh);
            }
        }
        HIP_TRY(per_knot ? launch_build_inst_lin_knots(q, s->stream) : launch_build_inst_lin(q, s->stream));
    }
    if (!in.fam()) {  // (the mode begins; the reference and clamp rows of every instance: this mode's kernel always reads them per instance)
        in.mark(0, s->batch);
        in.slopes_dirty = true;
    }
    in.lin = true;
    in.lin_nlx = nlx; in.lin_nlu = nlu; in.lin_nl = q.nl; in.lin_knots = q.knots;
    if (!s->layout_m) { in.fam_rows_nl = q.nl; in.fam_rows_knots = q.knots; }
    if (nlx != s->n_lin_x || nlu != s->n_lin_u) {  // (the shared rows are not read while the mode is on; they keep the handle's counts consistent)
        s->n_lin_x = nlx; s->n_lin_u = nlu;
        s->Alin_x.assign(ax, 0.0); s->blin_x.assign(nlx, std::numeric_limits<double>::infinity());
        s->Alin_u.assign(au, 0.0); s->blin_u.assign(nlu, std::numeric_limits<double>::infinity());
    }
    if (nlx > 0) s->st.en_state_linear = 1;  // as the shared verb
    if (nlu > 0) s->st.en_input_linear = 1;
    s->fam_dirty = true;
    // the caller keeps ownership of its buffers: everything has been read when the call returns (the tinympc_set_x0_batch_device rule)
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (old_rows) dfree(s, old_rows);
    return TINYMPC_OK;
}

// tinympc_set_cone_slopes_batch (+ _device): the cone slopes of instances [first, first+count) on the handle's cone structure. Host
// input is staged on the device; from there both forms are ONE path -- k_check_inst_slopes validates the values where they lie (one
// flag read back), then, and only then, k_store_inst_slopes copies them into the raw array every instance's slopes are kept in. The
// store the kernels read is rebuilt from it at the next launch (refresh_inst_families).
int set_cone_slopes_batch(tinympc_solver *s, const double *cx, int ncx, const double *cu, int ncu, bool on_device, int first, int count) {
    const char *verb = on_device ? "set_cone_slopes_batch_device" : "set_cone_slopes_batch";
    int rc = check_handle(s);
    if (rc) return rc;
    if (s->n_cone_x + s->n_cone_u == 0)
        return fail(TINYMPC_ERR_INVALID_INPUT, "%s: the handle holds no cones (tinympc_set_cone_constraints sets the structure)", verb);
    if (ncx != s->n_cone_x || ncu != s->n_cone_u)
        return fail(TINYMPC_ERR_INVALID_INPUT, "%s: %d state and %d input slopes, but the handle's structure has %d and %d cones", verb, ncx, ncu,
                    s->n_cone_x, s->n_cone_u);
    if ((ncx > 0 && !cx) || (ncu > 0 && !cu)) return fail(TINYMPC_ERR_INVALID_INPUT, "%s: NULL array for a non-empty side", verb);
    if (first < 0 || count < 1 || first > s->batch - count)
        return fail(TINYMPC_ERR_INVALID_INPUT, "%s: instance range [%d, %d + %d) is empty or outside batch of %d", verb, first, first, count, s->batch);
    if (on_device && ((ncx > 0 && !on_handles_device(s, cx)) || (ncu > 0 && !on_handles_device(s, cu))))
        return fail(TINYMPC_ERR_INVALID_INPUT, "%s: the slopes are not device memory of the handle's GPU %d", verb, s->device);
    InstState &in = s->inst;
    const size_t nc = (size_t)ncx + ncu, n = (size_t)count;
    if (s->batch == 1) {  // the shared verb with the held structure, after this verb's own checks of the values
        std::vector<double> h(nc);
        if (on_device && (rc = bind_device(s))) return rc;
        if (ncx > 0) { if (on_device) { if ((rc = download(s, h.data(), cx, sizeof(double) * ncx))) return rc; } else std::memcpy(h.data(), cx, sizeof(double) * ncx); }
        if (ncu > 0) { if (on_device) { if ((rc = download(s, h.data() + ncx, cu, sizeof(double) * ncu))) return rc; } else std::memcpy(h.data() + ncx, cu, sizeof(double) * ncu); }
        for (size_t i = 0; i < nc; ++i)
            if (!(h[i] > 0.0) || !std::isfinite(h[i])) return fail(TINYMPC_ERR_INVALID_INPUT, "%s: a slope is NaN, infinite or not positive", verb);
        const std::vector<int> Acx = s->Acx, qcx = s->qcx, Acu = s->Acu, qcu = s->qcu;
        const int esx = s->st.en_state_soc, esu = s->st.en_input_soc;
        rc = tinympc_set_cone_constraints(s, Acx.data(), qcx.data(), h.data(), ncx, Acu.data(), qcu.data(), h.data() + ncx, ncu);
        if (rc == TINYMPC_OK && (s->st.en_state_soc != esx || s->st.en_input_soc != esu)) {  // (this verb changes no enable flag)
            s->st.en_state_soc = esx; s->st.en_input_soc = esu;
        }
        return rc;
    }
    if ((rc = bind_device(s))) return rc;
    InstSlopeParams q{};
    q.W = s->W; q.ncx = ncx; q.ncu = ncu; q.batch = s->batch; q.groups = s->groups; q.first = first; q.count = count;
    q.cx_stride = (size_t)ncx; q.cu_stride = (size_t)ncu;
    double *old_stage = nullptr;
    if (on_device) {
        q.cx = cx; q.cu = cu;
    } else {
        if (nc * n > in.lstage_cap) {
            old_stage = in.lstage;
            if ((rc = dalloc(s, &in.lstage, nc * n))) return rc;
            in.lstage_cap = nc * n;
        }
        double *dcx = in.lstage, *dcu = dcx + (size_t)ncx * n;
        if (ncx > 0) HIP_TRY(hipMemcpyAsync(dcx, cx, sizeof(double) * ncx * n, hipMemcpyHostToDevice, s->stream));
        if (ncu > 0) HIP_TRY(hipMemcpyAsync(dcu, cu, sizeof(double) * ncu * n, hipMemcpyHostToDevice, s->stream));
        q.cx = dcx; q.cu = dcu;
    }
    if (!in.mflag && (rc = dalloc(s, &in.mflag, (size_t)1))) return rc;
    int bad = 0;
    HIP_TRY(hipMemsetAsync(in.mflag, 0, sizeof(int), s->stream));
    HIP_TRY(launch_check_inst_slopes(q, in.mflag, s->stream));
    if ((rc = download(s, &bad, in.mflag, sizeof(int)))) return rc;  // (host input has been copied when this returns)
    if (old_stage) dfree(s, old_stage);
    if (bad) return fail(TINYMPC_ERR_INVALID_INPUT, "%s: a slope is NaN, infinite or not positive", verb);
    // ---- valid: from here on the call writes
    if (nc * s->batch > in.craw_cap) {  // (a structure with more cones than the last one the half was on with; the half is off then)
        double *old = in.craw;
        if ((rc = dalloc(s, &in.craw, nc * s->batch))) return rc;
        in.craw_cap = nc * s->batch;
        if (old) dfree(s, old);
    }
    q.raw = in.craw; q.raw_stride = nc;
    if (!in.cones) {  // the half begins: every instance on the shared slopes of this moment
        if (!in.cshared && (rc = dalloc(s, &in.cshared, (size_t)HARD_MAX_CONES))) return rc;
        std::vector<double> h(s->cx);
        h.insert(h.end(), s->cu.begin(), s->cu.end());
        if ((rc = upload(s, in.cshared, h.data(), nc))) return rc;
        InstSlopeParams w = q;
        w.first = 0; w.count = s->batch;
        w.cx = in.cshared; w.cu = in.cshared + ncx; w.cx_stride = w.cu_stride = 0;
        HIP_TRY(launch_store_inst_slopes(w, s->stream));
    }
    HIP_TRY(launch_store_inst_slopes(q, s->stream));
    if (!in.fam()) {  // (the mode begins; the reference and clamp rows of every instance: its kernels always read them per instance)
        if (!s->layout_m && (rc = alloc_inst_rows(s, true))) return rc;
        in.mark(0, s->batch);
        in.shared_rows_dirty = true;
    }
    in.cones = true;
    in.slopes_dirty = true;
    // the caller keeps ownership of its buffers: everything has been read when the call returns (the tinympc_set_x0_batch_device rule)
    HIP_TRY(hipStreamSynchronize(s->stream));
    return TINYMPC_OK;
}

}  // namespace

int tinympc_set_cone_slopes_batch(tinympc_solver *s, const double *cx, int ncx, const double *cu, int ncu, int first, int count) {
    return set_cone_slopes_batch(s, cx, ncx, cu, ncu, false, first, count);
}
int tinympc_set_cone_slopes_batch_device(tinympc_solver *s, const double *d_cx, int ncx, const double *d_cu, int ncu, int first, int count) {
    return set_cone_slopes_batch(s, d_cx, ncx, d_cu, ncu, true, first, count);
}

int tinympc_set_linear_constraints_knots_batch(tinympc_solver *s, const double *Alin_x, const double *blin_x, int nlx, const double *Alin_u,
                                               const double *blin_u, int nlu, int first, int count) {
    return set_lin_batch(s, Alin_x, blin_x, nlx, Alin_u, blin_u, nlu, false, first, count, true);
}
int tinympc_set_linear_constraints_knots_batch_device(tinympc_solver *s, const double *d_Alin_x, const double *d_blin_x, int nlx, const double *d_Alin_u,
                                                      const double *d_blin_u, int nlu, int first, int count) {
    return set_lin_batch(s, d_Alin_x, d_blin_x, nlx, d_Alin_u, d_blin_u, nlu, true, first, count, true);
}
int tinympc_set_linear_constraints_batch(tinympc_solver *s, const double *Alin_x, const double *blin_x, int nlx, const double *Alin_u,
                                         const double *blin_u, int nlu, int first, int count) {
    return set_lin_batch(s, Alin_x, blin_x, nlx, Alin_u, blin_u, nlu, false, first, count);
}
int tinympc_set_linear_constraints_batch_device(tinympc_solver *s, const double *d_Alin_x, const double *d_blin_x, int nlx, const double *d_Alin_u,
                                                const double *d_blin_u, int nlu, int first, int count) {
    return set_lin_batch(s, d_Alin_x, d_blin_x, nlx, d_Alin_u, d_blin_u, nlu, true, first, count);
}

int tinympc_set_model_batch(tinympc_solver *s, const double *A, const double *B, const double *fdyn, const double *Q, const double *R,
                            int first, int count) {
    return set_model_batch(s, A, B, fdyn, Q, R, false, first, count);
}
int tinympc_set_model_batch_device(tinympc_solver *s, const double *d_A, const double *d_B, const double *d_fdyn, const double *d_Q,
                                   const double *d_R, int first, int count) {
    return set_model_batch(s, d_A, d_B, d_fdyn, d_Q, d_R, true, first, count);
}

int tinympc_set_rho_batch(tinympc_solver *s, const double *rho, int first, int count) { return set_rho_batch(s, rho, false, first, count); }
int tinympc_set_rho_batch_device(tinympc_solver *s, const double *d_rho, int first, int count) { return set_rho_batch(s, d_rho, true, first, count); }

int tinympc_clear_model_batch(tinympc_solver *s) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (!s->inst.models) return TINYMPC_OK;
    s->inst.models = false;
    s->inst.rho_verb = false;  // (and every instance is back on the shared rho)
    // the rows that stay in use (per-instance references / bounds) are built from the shared Pinf and cost diagonals again
    if (s->inst_tables()) s->inst.mark(0, s->batch);
    return TINYMPC_OK;
}

int tinympc_get_cache_batch(tinympc_solver *s, double *Kinf, double *Pinf, double *Quu_inv, double *AmBKt, int *riccati_iters,
                            int first, int count) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (first < 0 || count < 0 || first + count > s->batch)
        return fail(TINYMPC_ERR_INVALID_INPUT, "get_cache_batch: instance range [%d, %d) outside batch of %d", first, first + count, s->batch);
    if ((rc = bind_device(s))) return rc;
    const size_t nx = s->nx, nu = s->nu, n = (size_t)count;
    const InstState &in = s->inst;
    if (in.models && in.ops) {
        if (Kinf && (rc = download(s, Kinf, in.cK + first * nu * nx, sizeof(double) * nu * nx * n))) return rc;
        if (Pinf && (rc = download(s, Pinf, in.cP + first * nx * nx, sizeof(double) * nx * nx * n))) return rc;
        if (Quu_inv && (rc = download(s, Quu_inv, in.cQuu + first * nu * nu, sizeof(double) * nu * nu * n))) return rc;
        if (AmBKt && (rc = download(s, AmBKt, in.cAm + first * nx * nx, sizeof(double) * nx * nx * n))) return rc;
        if (riccati_iters) {
            std::vector<int> info(4 * n);
            if (n && (rc = download(s, info.data(), in.cinfo + (size_t)first * 4, sizeof(int) * 4 * n))) return rc;
            for (size_t b = 0; b < n; ++b) riccati_iters[b] = info[4 * b];
        }
        return TINYMPC_OK;
    }
    // without per-instance models: the shared cache, repeated
    if (n == 0) return TINYMPC_OK;
    int it = 0;
    if ((rc = tinympc_get_cache(s, Kinf, Pinf, Quu_inv, AmBKt, riccati_iters ? &it : nullptr))) return rc;
    for (size_t b = 1; b < n; ++b) {
        if (Kinf) std::memcpy(Kinf + b * nu * nx, Kinf, sizeof(double) * nu * nx);
        if (Pinf) std::memcpy(Pinf + b * nx * nx, Pinf, sizeof(double) * nx * nx);
        if (Quu_inv) std::memcpy(Quu_inv + b * nu * nu, Quu_inv, sizeof(double) * nu * nu);
        if (AmBKt) std::memcpy(AmBKt + b * nx * nx, AmBKt, sizeof(double) * nx * nx);
    }
    for (size_t b = 0; riccati_iters && b < n; ++b) riccati_iters[b] = it;
    return TINYMPC_OK;
}

int tinympc_reset_workspace(tinympc_solver *s) {
    int rc = check_handle(s);
    if (rc) return rc;
    if ((rc = bind_device(s))) return rc;
    // G, V, D: zero by CONTRACT from here on, written to HBM only if the next kernel needs them there (materialize_cold_state):
    // the throughput kernel starts a cold solve from zero registers instead of loading 14 KB of zeros per instance that a
    // memset would have had to write first (119 MB per 8,192 quadrotor instances, ~35 us of a 1.86 ms step).
    // (V2, the stale-copy buffer of layout B, and LX, the families' forward -> backward term, are always written
    //  before they are read within a solve: nothing to reset)
    s->cold_state = true;
    if (s->dGC) {
        HIP_TRY(hipMemsetAsync(s->dGC, 0, sizeof(double) * s->v_doubles(), s->stream));
        HIP_TRY(hipMemsetAsync(s->dGL, 0, sizeof(double) * s->v_doubles(), s->stream));
    }
    s->sol_zero_pending = true;  // (sol_x / sol_u: zero by contract; the next solve overwrites them, a reader before that gets zeros written first)
    if (s->sol_ptrs_exported && (rc = materialize_zero_solution(s))) return rc;  // ... a reader that holds the device pointers comes through no verb
    HIP_TRY(launch_reset_stats(s->distats, s->ddstats, s->drho_inst, s->batch, s->rho, s->stream));  // (adapted rho back to the setup value)
    s->host_sol_state = 0;  // the device solution / statistics were just zeroed: read them from there
    return TINYMPC_OK;
}

int tinympc_get_rho_batch(tinympc_solver *s, double *rho_out, int first, int count) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (!rho_out || first < 0 || count < 0 || first + count > s->batch)
        return fail(TINYMPC_ERR_INVALID_INPUT, "get_rho_batch: range [%d, %d) outside the batch of %d", first, first + count, s->batch);
    if ((rc = bind_device(s))) return rc;
    // (per-instance models: the instance's own rho, which reset_workspace keeps; otherwise the adaptive-rho value / the setup value)
    const double *src = (s->inst.models && s->inst.mrho) ? s->inst.mrho : s->drho_inst;
    return download(s, rho_out, src + first, sizeof(double) * count);
}

int tinympc_get_solution_device_ptrs(tinympc_solver *s, const double **d_x, const double **d_u) {
    int rc = check_handle(s);
    if (rc) return rc;
    if ((rc = bind_device(s))) return rc;
    if ((rc = materialize_zero_solution(s))) return rc;
    s->sol_ptrs_exported = true;  // from here on tinympc_reset_workspace zeroes the buffers itself instead of deferring it
    if (d_x) *d_x = s->dsolx;
    if (d_u) *d_u = s->dsolu;
    return TINYMPC_OK;
}


// ---- closed-loop rollout on the device (k_plant_step, tinympc_rollout.hip)
namespace {

// A buffer of the rollout's host form: grown to `need` elements where it is smaller, otherwise left alone (never shrunk).
extern "C++" template <typename T>
int grow_rollout_buffer(tinympc_solver *s, T **p, size_t *cap, size_t need) {
    if (need <= *cap && *p) return TINYMPC_OK;
    dfree(s, *p);
    *p = nullptr;
    *cap = 0;
    int rc = dalloc(s, p, need);
    if (rc) return rc;
    *cap = need;
    return TINYMPC_OK;
}

// The plant of a step: the override, else the instance's own model while per-instance models are on, else the shared model.
void fill_plant_operands(const tinympc_solver *s, PlantStepParams *p) {
    const size_t nx = s->nx, nu = s->nu;
    if (s->plant) {
        p->A = s->pA; p->B = s->pB; p->f = s->pf;
        p->A_stride = nx * nx; p->B_stride = nx * nu; p->f_stride = nx;
    } else if (s->inst.models) {
        p->A = s->inst.mA; p->B = s->inst.mB; p->f = s->inst.mf;
        p->A_stride = nx * nx; p->B_stride = nx * nu; p->f_stride = nx;
    } else {
        p->A = s->dA; p->B = s->dB; p->f = s->dfdyn;
        p->A_stride = p->B_stride = p->f_stride = 0;
    }
    p->nx = s->nx; p->nu = s->nu; p->batch = s->batch;
    p->u_stride = s->U();
    p->x0 = s->dx0; p->sol_u = s->dsolu; p->istats = s->distats;
}

// What the scored step measures against: the reference and the bounds the solve itself used at knot 0. A half in track mode: the
// instance's column min(steps[b], T - 1) of its track (the kernel reads the step: the step of THIS tick, the auto-advance comes behind
// it); else the instance's own reference, column 0; else the shared one. Bounds: the instance's where that mode is on, else the shared
// ones; NULL while the family is disabled (the slot stays 0).
void fill_metrics_operands(const tinympc_solver *s, PlantMetricsParams *q) {
    const InstState &in = s->inst;
    const size_t nx = s->nx, nu = s->nu, X = s->X(), U = s->U();
    *q = PlantMetricsParams{};
    q->rows = s->rm_rows; q->qx = s->rm_w; q->ru = s->rm_w + nx; q->settle_tol = s->rm_tol;
    q->steps = in.steps;
    if (in.x && in.x_track && in.Xt && in.steps) { q->xr = in.Xt; q->xr_stride = nx * (size_t)in.Tx; q->xr_T = in.Tx; }
    else if (in.x && in.Xi) { q->xr = in.Xi; q->xr_stride = X; }
    else { q->xr = s->dXref; q->xr_stride = 0; }
    if (in.u && in.u_track && in.Ut && in.steps) { q->ur = in.Ut; q->ur_stride = nu * (size_t)in.Tu; q->ur_T = in.Tu; }
    else if (in.u && in.Ui) { q->ur = in.Ui; q->ur_stride = U; }
    else { q->ur = s->dUref; q->ur_stride = 0; }
    const bool ib = in.bounds && in.xmin && in.xmax && in.umin && in.umax;
    if (s->st.en_state_bound) { q->xlo = ib ? in.xmin : s->dxmin; q->xhi = ib ? in.xmax : s->dxmax; q->xb_stride = ib ? X : 0; }
    if (s->st.en_input_bound) { q->ulo = ib ? in.umin : s->dumin; q->uhi = ib ? in.umax : s->dumax; q->ub_stride = ib ? U : 0; }
}

// The noise operands of a step (or of a replay) at `tick`: the key, the scales of the families that are on, the true state beside x0.
void fill_noise_operands(const tinympc_solver *s, unsigned long long tick, PlantNoiseParams *n) {
    *n = PlantNoiseParams{};
    n->key0 = (unsigned)(s->rn_seed & 0xffffffffull); n->key1 = (unsigned)(s->rn_seed >> 32);
    n->tick = (unsigned)tick;
    n->first_instance = s->rn_first;
    if (s->rn_w_on) { n->sw = s->rn_sw; n->sw_stride = s->rn_stride; }
    if (s->rn_v_on) { n->sv = s->rn_sv; n->sv_stride = s->rn_stride; n->px = s->rn_px; }
}

// What a verb that queues `steps` plant steps refuses while the noise is on: a tick is 32 bits of the draw's counter.
int noise_tick_refusal(const tinympc_solver *s, const char *verb, unsigned long long steps) {
    if (s->noise && s->rn_tick + steps > (1ull << 32))
        return fail(TINYMPC_ERR_INVALID_INPUT, "%s: the rollout noise is at tick %llu, and %llu more would reach 2^32 (tinympc_set_rollout_noise starts again at 0)",
                    verb, s->rn_tick, steps);
    return TINYMPC_OK;
}

// One plant step on the handle's stream: the scored variant while the metrics are on, the plain kernel otherwise; the noisy variant of
// either while the rollout noise is on, at the handle's noise tick, which moves on by one.
int queue_plant_step(tinympc_solver *s, const PlantStepParams &p) {
    if (s->noise) {
        PlantMetricsParams q;
        PlantNoiseParams n;
        if (s->metrics) fill_metrics_operands(s, &q);
        fill_noise_operands(s, s->rn_tick, &n);
        HIP_TRY(launch_plant_step_noisy(p, s->metrics ? &q : nullptr, n, s->W, s->KT, s->stream));
        ++s->rn_tick;
    } else if (s->metrics) {
        PlantMetricsParams q;
        fill_metrics_operands(s, &q);
        HIP_TRY(launch_plant_step_scored(p, q, s->W, s->KT, s->stream));
    } else {
        HIP_TRY(launch_plant_step(p, s->W, s->KT, s->stream));
    }
    return TINYMPC_OK;
}

// What both forms of the rollout refuse, before anything is queued or changed; on success the device is bound and the plan resolved.
int rollout_refusals(tinympc_solver *s, const char *verb, int ticks) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (ticks < 1) return fail(TINYMPC_ERR_INVALID_INPUT, "%s: ticks must be >= 1 (got %d)", verb, ticks);
    if (s->session_active || s->host_path()) return fail(TINYMPC_ERR_UNSUPPORTED, "%s: batched handles outside a session only", verb);
    if (s->st.max_iter < 1)
        return fail(TINYMPC_ERR_INVALID_INPUT, "%s: max_iter must be >= 1 (a tick of %d iterations writes no control to roll out)", verb, s->st.max_iter);
    if ((rc = noise_tick_refusal(s, verb, (unsigned long long)ticks))) return rc;
    if ((rc = bind_device(s))) return rc;
    if ((rc = resolve_plan(s))) return rc;  // (a run-time specialisation happens here, outside the queue)
    return check_launch(s, current_plan(s));  // (the launch's own refusal, with its message)
}

// ticks x (what a tinympc_mpc_step_batch tick launches, x0 read from dx0; k_plant_step; the tracks' auto-advance) on the handle's
// stream: no copy, no synchronisation, no graph.
int queue_rollout(tinympc_solver *s, int ticks, const double *d_w, const tinympc_rollout_logs &d_logs) {
    int rc;
    PlantStepParams p{};
    p.ticks = ticks;
    p.w = d_w;
    p.x_log = d_logs.x_log; p.u_log = d_logs.u_log; p.iter_log = d_logs.iter_log; p.status_log = d_logs.status_log;
    for (int t = 0; t < ticks; ++t) {
        if ((rc = refresh_derived(s))) return rc;
        if ((rc = refresh_inst_tables(s))) return rc;
        if ((rc = launch(s, false))) return rc;
        fill_plant_operands(s, &p);
        p.t = t;
        if ((rc = queue_plant_step(s, p))) return rc;
        if (s->inst.auto_advance && (rc = advance_ref_steps_after_tick(s))) return rc;
    }
    return TINYMPC_OK;
}

// tinympc_set_plant_batch (+ _device)
int set_plant_batch(tinympc_solver *s, const double *A, const double *B, const double *f, bool on_device, int first, int count) {
    const char *verb = on_device ? "set_plant_batch_device" : "set_plant_batch";
    int rc = check_handle(s);
    if (rc) return rc;
    if (!A || !B) return fail(TINYMPC_ERR_INVALID_INPUT, "%s requires A and B", verb);
    if (first < 0 || count < 1 || first + count > s->batch)
        return fail(TINYMPC_ERR_INVALID_INPUT, "%s: instance range [%d, %d) is empty or outside batch of %d", verb, first, first + count, s->batch);
    if (s->session_active || s->host_path()) return fail(TINYMPC_ERR_UNSUPPORTED, "%s: batched handles outside a session only", verb);
    if (!s->plant && (first != 0 || count != s->batch))
        return fail(TINYMPC_ERR_INVALID_INPUT, "%s: the first call must name the whole batch (got [%d, %d) of %d)", verb, first, first + count, s->batch);
    const size_t nx = s->nx, nu = s->nu, n = (size_t)count, batch = (size_t)s->batch;
    if (on_device) {
        if (!on_handles_device(s, A) || !on_handles_device(s, B) || (f && !on_handles_device(s, f)))
            return fail(TINYMPC_ERR_INVALID_INPUT, "%s: the plant is not device memory of the handle's GPU %d", verb, s->device);
        if ((rc = bind_device(s))) return rc;
        InstState &in = s->inst;
        if (!in.mflag && (rc = dalloc(s, &in.mflag, (size_t)1))) return rc;
        int bad = 0;
        HIP_TRY(hipMemsetAsync(in.mflag, 0, sizeof(int), s->stream));
        HIP_TRY(launch_check_finite(A, nx * nx * n, in.mflag, s->stream));
        HIP_TRY(launch_check_finite(B, nx * nu * n, in.mflag, s->stream));
        if (f) HIP_TRY(launch_check_finite(f, nx * n, in.mflag, s->stream));
        if ((rc = download(s, &bad, in.mflag, sizeof(int)))) return rc;
        if (bad) return fail(TINYMPC_ERR_INVALID_INPUT, "%s: every entry of the plant must be finite", verb);
    } else {
        const double *arr[3] = {A, B, f};
        const size_t len[3] = {nx * nx * n, nx * nu * n, nx * n};
        const char *name[3] = {"A", "B", "f"};
        for (int a = 0; a < 3; ++a)
            for (size_t i = 0; arr[a] && i < len[a]; ++i)
                if (!std::isfinite(arr[a][i])) return fail(TINYMPC_ERR_INVALID_INPUT, "%s: %s[%zu] = %g. Expected a finite number.", verb, name[a], i, arr[a][i]);
        if ((rc = bind_device(s))) return rc;
    }
    if (!s->pA && ((rc = dalloc(s, &s->pA, nx * nx * batch)) || (rc = dalloc(s, &s->pB, nx * nu * batch)) || (rc = dalloc(s, &s->pf, nx * batch)))) return rc;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    HIP_TRY(hipMemcpyAsync(s->pA + (size_t)first * nx * nx, A, sizeof(double) * nx * nx * n, kind, s->stream));
    HIP_TRY(hipMemcpyAsync(s->pB + (size_t)first * nx * nu, B, sizeof(double) * nx * nu * n, kind, s->stream));
    if (f) HIP_TRY(hipMemcpyAsync(s->pf + (size_t)first * nx, f, sizeof(double) * nx * n, kind, s->stream));
    else HIP_TRY(hipMemsetAsync(s->pf + (size_t)first * nx, 0, sizeof(double) * nx * n, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));  // (the caller keeps ownership of its buffers: copied when the call returns)
    s->plant = true;
    return TINYMPC_OK;
}

}  // namespace

int tinympc_rollout_batch(tinympc_solver *s, int ticks, const double *disturbance, const tinympc_rollout_logs *logs, float *gpu_ms) {
    int rc = rollout_refusals(s, "rollout_batch", ticks);
    if (rc) return rc;
    const size_t nx = s->nx, nu = s->nu, batch = s->batch, T = (size_t)ticks;
    const tinympc_rollout_logs want = logs ? *logs : tinympc_rollout_logs{nullptr, nullptr, nullptr, nullptr};
    tinympc_rollout_logs d{nullptr, nullptr, nullptr, nullptr};
    if (want.x_log) { if ((rc = grow_rollout_buffer(s, &s->rl_x, &s->rl_x_cap, nx * (T + 1) * batch))) return rc; d.x_log = s->rl_x; }
    if (want.u_log) { if ((rc = grow_rollout_buffer(s, &s->rl_u, &s->rl_u_cap, nu * T * batch))) return rc; d.u_log = s->rl_u; }
    if (want.iter_log) { if ((rc = grow_rollout_buffer(s, &s->rl_it, &s->rl_it_cap, T * batch))) return rc; d.iter_log = s->rl_it; }
    if (want.status_log) { if ((rc = grow_rollout_buffer(s, &s->rl_st, &s->rl_st_cap, T * batch))) return rc; d.status_log = s->rl_st; }
    if (disturbance) {
        if ((rc = grow_rollout_buffer(s, &s->rl_w, &s->rl_w_cap, nx * T * batch))) return rc;
        if ((rc = upload(s, s->rl_w, disturbance, nx * T * batch))) return rc;
    }
    if (gpu_ms) HIP_TRY(hipEventRecord(s->ev0, s->stream));
    if ((rc = queue_rollout(s, ticks, disturbance ? s->rl_w : nullptr, d))) return rc;
    if (gpu_ms) HIP_TRY(hipEventRecord(s->ev1, s->stream));
    // the one synchronisation of the rollout, then the requested logs
    if (d.x_log) HIP_TRY(hipMemcpyAsync(want.x_log, d.x_log, sizeof(double) * nx * (T + 1) * batch, hipMemcpyDeviceToHost, s->stream));
    if (d.u_log) HIP_TRY(hipMemcpyAsync(want.u_log, d.u_log, sizeof(double) * nu * T * batch, hipMemcpyDeviceToHost, s->stream));
    if (d.iter_log) HIP_TRY(hipMemcpyAsync(want.iter_log, d.iter_log, sizeof(int) * T * batch, hipMemcpyDeviceToHost, s->stream));
    if (d.status_log) HIP_TRY(hipMemcpyAsync(want.status_log, d.status_log, sizeof(int) * T * batch, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (gpu_ms) HIP_TRY(hipEventElapsedTime(gpu_ms, s->ev0, s->ev1));
    return TINYMPC_OK;
}

int tinympc_rollout_batch_device(tinympc_solver *s, int ticks, const double *d_disturbance, const tinympc_rollout_logs *d_logs) {
    int rc = check_handle(s);
    if (rc) return rc;
    const tinympc_rollout_logs d = d_logs ? *d_logs : tinympc_rollout_logs{nullptr, nullptr, nullptr, nullptr};
    const void *ptrs[5] = {d_disturbance, d.x_log, d.u_log, d.iter_log, d.status_log};
    for (const void *q : ptrs)
        if (q && !on_handles_device(s, q))
            return fail(TINYMPC_ERR_INVALID_INPUT, "rollout_batch_device: the disturbance and the logs must be device memory of the handle's GPU %d", s->device);
    if ((rc = rollout_refusals(s, "rollout_batch_device", ticks))) return rc;
    return queue_rollout(s, ticks, d_disturbance, d);
}

int tinympc_plant_step_batch(tinympc_solver *s, const double *disturbance) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (s->session_active || s->host_path()) return fail(TINYMPC_ERR_UNSUPPORTED, "plant_step_batch: batched handles outside a session only");
    if ((rc = noise_tick_refusal(s, "plant_step_batch", 1))) return rc;
    if ((rc = bind_device(s))) return rc;
    if ((rc = materialize_zero_solution(s))) return rc;  // (no solve since a reset: the first controls are zeros)
    const size_t n = (size_t)s->nx * s->batch;
    if (disturbance) {
        if ((rc = grow_rollout_buffer(s, &s->rl_w, &s->rl_w_cap, n))) return rc;
        if ((rc = upload(s, s->rl_w, disturbance, n))) return rc;
    }
    PlantStepParams p{};
    fill_plant_operands(s, &p);
    p.t = 0; p.ticks = 1;
    p.w = disturbance ? s->rl_w : nullptr;
    return queue_plant_step(s, p);
}

int tinympc_set_plant_batch(tinympc_solver *s, const double *A, const double *B, const double *f, int first, int count) {
    return set_plant_batch(s, A, B, f, false, first, count);
}
int tinympc_set_plant_batch_device(tinympc_solver *s, const double *d_A, const double *d_B, const double *d_f, int first, int count) {
    return set_plant_batch(s, d_A, d_B, d_f, true, first, count);
}

int tinympc_clear_plant_batch(tinympc_solver *s) {
    int rc = check_handle(s);
    if (rc) return rc;
    s->plant = false;  // (the stores stay for the next override)
    return TINYMPC_OK;
}

// ---- rollout metrics (the scored variant of k_plant_step)
namespace {

// What every metrics verb refuses first; `need_on`: the verbs that read or zero the rows want the metrics on.
int metrics_refusals(const tinympc_solver *s, const char *verb, bool need_on) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (s->session_active || s->host_path()) return fail(TINYMPC_ERR_UNSUPPORTED, "%s: batched handles outside a session only", verb);
    if (need_on && !s->metrics)
        return fail(TINYMPC_ERR_INVALID_INPUT, "%s: the rollout metrics are off (tinympc_set_rollout_metrics turns them on)", verb);
    return TINYMPC_OK;
}

}  // namespace

int tinympc_set_rollout_metrics(tinympc_solver *s, const tinympc_rollout_score *score) {
    const char *verb = "set_rollout_metrics";
    int rc = metrics_refusals(s, verb, false);
    if (rc) return rc;
    if (!score || !score->qx || !score->ru) return fail(TINYMPC_ERR_INVALID_INPUT, "%s requires qx and ru", verb);
    const size_t nx = s->nx, nu = s->nu;
    for (size_t i = 0; i < nx + nu; ++i) {
        const double v = i < nx ? score->qx[i] : score->ru[i - nx];
        if (!std::isfinite(v) || v < 0.0)
            return fail(TINYMPC_ERR_INVALID_INPUT, "%s: %s[%zu] = %g. Expected a finite weight >= 0.", verb, i < nx ? "qx" : "ru", i < nx ? i : i - nx, v);
    }
    if (!std::isfinite(score->settle_tol)) return fail(TINYMPC_ERR_INVALID_INPUT, "%s: settle_tol = %g. Expected a finite number.", verb, score->settle_tol);
    if ((rc = bind_device(s))) return rc;
    if (!s->rm_rows && (rc = dalloc(s, &s->rm_rows, (size_t)8 * s->batch))) return rc;
    if (!s->rm_w && (rc = dalloc(s, &s->rm_w, nx + nu))) return rc;
    std::vector<double> w(nx + nu);
    for (size_t i = 0; i < nx + nu; ++i) w[i] = i < nx ? score->qx[i] : score->ru[i - nx];
    HIP_TRY(hipMemsetAsync(s->rm_rows, 0, sizeof(double) * 8 * s->batch, s->stream));
    if ((rc = upload(s, s->rm_w, w.data(), nx + nu))) return rc;  // (behind every step queued so far: they read the weights they were queued with)
    s->rm_tol = score->settle_tol;
    s->metrics = true;
    return TINYMPC_OK;
}

int tinympc_reset_rollout_metrics(tinympc_solver *s) {
    int rc = metrics_refusals(s, "reset_rollout_metrics", true);
    if (rc) return rc;
    if ((rc = bind_device(s))) return rc;
    HIP_TRY(hipMemsetAsync(s->rm_rows, 0, sizeof(double) * 8 * s->batch, s->stream));
    return TINYMPC_OK;
}

int tinympc_clear_rollout_metrics(tinympc_solver *s) {
    int rc = metrics_refusals(s, "clear_rollout_metrics", false);
    if (rc) return rc;
    s->metrics = false;  // (the rows and the weights stay for the next call of tinympc_set_rollout_metrics, which zeroes the rows)
    return TINYMPC_OK;
}

int tinympc_get_rollout_metrics(tinympc_solver *s, double *out) {
    int rc = metrics_refusals(s, "get_rollout_metrics", true);
    if (rc) return rc;
    if (!out) return fail(TINYMPC_ERR_INVALID_INPUT, "get_rollout_metrics: out is NULL");
    if ((rc = bind_device(s))) return rc;
    return download(s, out, s->rm_rows, sizeof(double) * 8 * s->batch);
}

int tinympc_get_rollout_metrics_device_ptr(tinympc_solver *s, const double **d_rows) {
    int rc = metrics_refusals(s, "get_rollout_metrics_device_ptr", true);
    if (rc) return rc;
    if (!d_rows) return fail(TINYMPC_ERR_INVALID_INPUT, "get_rollout_metrics_device_ptr: d_rows is NULL");
    *d_rows = s->rm_rows;
    return TINYMPC_OK;
}

// ---- rollout noise (the noisy variants of k_plant_step; the draw: tinympc_rollout_noise.h)
namespace {

int noise_refusals(const tinympc_solver *s, const char *verb, bool need_on) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (s->session_active || s->host_path()) return fail(TINYMPC_ERR_UNSUPPORTED, "%s: batched handles outside a session only", verb);
    if (need_on && !s->noise)
        return fail(TINYMPC_ERR_INVALID_INPUT, "%s: the rollout noise is off (tinympc_set_rollout_noise turns it on)", verb);
    return TINYMPC_OK;
}

// x0 <- the true state, queued: what ends measurement noise, so that the loop goes on from the state the plant carries
int px_back_into_x0(tinympc_solver *s) {
    HIP_TRY(hipMemcpyAsync(s->dx0, s->rn_px, sizeof(double) * s->nx * s->batch, hipMemcpyDeviceToDevice, s->stream));
    return TINYMPC_OK;
}

}  // namespace

int tinympc_set_rollout_noise(tinympc_solver *s, const tinympc_rollout_noise *noise) {
    const char *verb = "set_rollout_noise";
    int rc = noise_refusals(s, verb, false);
    if (rc) return rc;
    if (!noise || (!noise->process && !noise->measurement)) return fail(TINYMPC_ERR_INVALID_INPUT, "%s requires process or measurement scales", verb);
    const size_t nx = s->nx, batch = s->batch, n = noise->per_instance ? nx * batch : nx;
    for (int a = 0; a < 2; ++a) {
        const double *v = a ? noise->measurement : noise->process;
        for (size_t i = 0; v && i < n; ++i)
            if (!std::isfinite(v[i]) || v[i] < 0.0)
                return fail(TINYMPC_ERR_INVALID_INPUT, "%s: %s[%zu] = %g. Expected a finite standard deviation >= 0.", verb, a ? "measurement" : "process", i, v[i]);
    }
    if (noise->first_instance > (1ull << 32) || noise->first_instance + batch > (1ull << 32))
        return fail(TINYMPC_ERR_INVALID_INPUT, "%s: first_instance %llu + batch %zu is beyond 2^32 (a global index is 32 bits of the draw's counter)",
                    verb, noise->first_instance, batch);
    if ((rc = bind_device(s))) return rc;
    if (noise->process && !s->rn_sw && (rc = dalloc(s, &s->rn_sw, nx * batch))) return rc;
    if (noise->measurement && !s->rn_sv && (rc = dalloc(s, &s->rn_sv, nx * batch))) return rc;
    if (noise->measurement && !s->rn_px && (rc = dalloc(s, &s->rn_px, nx * batch))) return rc;
    // (behind every step queued so far: they drew with the scales they were queued with)
    if (noise->process && (rc = upload(s, s->rn_sw, noise->process, n))) return rc;
    if (noise->measurement && (rc = upload(s, s->rn_sv, noise->measurement, n))) return rc;
    const bool had_px = s->noise && s->rn_v_on;
    if (had_px && !noise->measurement && (rc = px_back_into_x0(s))) return rc;
    s->noise = true;
    s->rn_w_on = noise->process != nullptr;
    s->rn_v_on = noise->measurement != nullptr;
    s->rn_stride = noise->per_instance ? nx : 0;
    s->rn_seed = noise->seed; s->rn_first = noise->first_instance; s->rn_tick = 0;
    if (!had_px) return mirror_x0_into_px(s, 0, s->batch);  // measurement noise just turned on: the true state is what x0 holds
    return TINYMPC_OK;
}

int tinympc_clear_rollout_noise(tinympc_solver *s) {
    int rc = noise_refusals(s, "clear_rollout_noise", true);
    if (rc) return rc;
    if (s->rn_v_on) {
        if ((rc = bind_device(s))) return rc;
        if ((rc = px_back_into_x0(s))) return rc;
    }
    s->noise = s->rn_w_on = s->rn_v_on = false;  // (the scales and px stay allocated for the next call of tinympc_set_rollout_noise)
    return TINYMPC_OK;
}

int tinympc_get_rollout_noise(tinympc_solver *s, unsigned long long first_tick, int ticks, double *w_out, double *v_out) {
    const char *verb = "get_rollout_noise";
    int rc = noise_refusals(s, verb, true);
    if (rc) return rc;
    if (ticks < 1) return fail(TINYMPC_ERR_INVALID_INPUT, "%s: ticks must be >= 1 (got %d)", verb, ticks);
    if (first_tick > (1ull << 32) || first_tick + (unsigned long long)ticks > (1ull << 32))
        return fail(TINYMPC_ERR_INVALID_INPUT, "%s: ticks [%llu, %llu + %d) reach 2^32", verb, first_tick, first_tick, ticks);
    if (!w_out && !v_out) return TINYMPC_OK;
    if ((rc = bind_device(s))) return rc;
    const size_t n = (size_t)s->nx * (size_t)ticks * s->batch;
    if ((rc = grow_rollout_buffer(s, &s->rn_out, &s->rn_out_cap, 2 * n))) return rc;
    PlantNoiseParams q;
    fill_noise_operands(s, first_tick, &q);
    HIP_TRY(launch_rollout_noise(q, s->nx, s->batch, ticks, w_out ? s->rn_out : nullptr, v_out ? s->rn_out + n : nullptr, s->stream));
    if (w_out) HIP_TRY(hipMemcpyAsync(w_out, s->rn_out, sizeof(double) * n, hipMemcpyDeviceToHost, s->stream));
    if (v_out) HIP_TRY(hipMemcpyAsync(v_out, s->rn_out + n, sizeof(double) * n, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return TINYMPC_OK;
}

int tinympc_get_plant_state_batch(tinympc_solver *s, double *x_out) {
    int rc = noise_refusals(s, "get_plant_state_batch", false);
    if (rc) return rc;
    if (!x_out) return fail(TINYMPC_ERR_INVALID_INPUT, "get_plant_state_batch: x_out is NULL");
    if ((rc = bind_device(s))) return rc;
    return download(s, x_out, s->noise && s->rn_v_on ? s->rn_px : s->dx0, sizeof(double) * s->nx * s->batch);
}

#ifdef TINY_CLOCK_STAMP
// Diagnostic build only (not part of the ABI): the stamp records of the last layout-D launch, 8 values per wavefront (see the
// kernel); returns the number of wavefronts copied into records[8 * capacity].
int tinympc_debug_clock_stamps(tinympc_solver *s, unsigned long long *records, int capacity) {
    if (!s || !s->dclock) return 0;
    if (hipSetDevice(s->device) != hipSuccess || hipStreamSynchronize(s->stream) != hipSuccess) return 0;
    const int n = s->groups < capacity ? s->groups : capacity;
    if (hipMemcpy(records, s->dclock, sizeof(unsigned long long) * 8 * n, hipMemcpyDeviceToHost) != hipSuccess) return 0;
    return n;
}
#endif

void *tinympc_get_stream(tinympc_solver *s) { return s ? (void *)s->stream : nullptr; }

}  // extern "C"
