// tinympc_rollout.hip -- k_plant_step: the plant behind a closed-loop tick's solve, on the handle's stream (tinympc_rollout_batch,
// tinympc_rollout_batch_device, tinympc_plant_step_batch). Every instance's measured state moves on the device,
//     x+ = A_p x + B_p u + f_p + w,      x = x0[b], u = the first control of the solve that just ran,
// and the tick's x, u, iteration count and status go to the logs (PlantStepParams, tinympc_rollout.h). No solve kernel is touched: the
// step reads what a solve leaves in sol_u / istats and writes what the next one reads from x0.
//
// Summation order (fixed; the tests pin the rollout to single steps bit for bit, and to numpy within rounding): ONE chain of fused
// multiply-adds per row, starting from f_p[r] (zeros where the plant has no affine term), over A's columns ascending, continued over
// B's columns ascending; then + w[r] (skipped without a disturbance). The wavefront form pads the chain to the handle's operand
// length KT with products of exact zeros.
//
// Wavefront form (nx+nu <= 64): the handle's own lanes per instance (W = 16 / 32 / 64), row r of x+ in lane r. The operand vector
// x | u sits one entry per lane and reaches the other lanes of the instance through the sweeps' fused DPP chain (group_matvec,
// tinympc_sweep.h: row_newbcast inside a 16-lane row, the cross-row swaps for the wide shapes; the chain opens with the two wait
// states a DPP read of a just-written register needs, and this object is linted for it like the solve kernels). A and B are read
// column by column: consecutive lanes read consecutive doubles. An instance lives in one wavefront, whose loads of x0 have all
// retired before the chain runs and therefore before any of its lanes stores x+.
// Workgroup form (nx+nu > 64, layout M's systems): one workgroup per instance, x | u staged in LDS, a barrier, then the same chain per
// row with plain v_fma_f64 -- every read of x0 is behind the barrier before the first store.
// Lanes beyond the batch and rows beyond nx load nothing and store nothing. Plain vector stores only.
//
// Scored variant (k_plant_step_scored<W, KT>, k_plant_step_wg_scored; PlantMetricsParams in tinympc_rollout.h): the same text compiled
// with PLANT_SCORED (tinympc_rollout_body.h) moves every instance's metrics row on as well. Lane r forms its row's term
// qx_r (e_r e_r) / ru_j (d_j d_j) and its breach of the bounds. The cost is ONE more group_matvec chain, over a matrix of ones, started
// from the stored cost in lane 1 (the lane of slot 1): state rows ascending, then input rows, padding lanes adding exact zeros --
// fma(1, term, acc) rounds once, so the chain IS the sequential sum of the documented order. The three maxima are group_max (any
// order: max is exact). Lanes 0..7 of the instance then read, update and store one slot each: one 64-byte line per instance. The
// workgroup form leaves the terms in LDS behind the barrier the plant has anyway; thread 0 runs the same sum and the maxima.
// No atomics, no scratch; x0 and the logs get the bits of the plain kernel.
//
// Noisy variants (k_plant_step_noisy<W, KT>, k_plant_step_wg_noisy and the scored-and-noisy pair; PlantNoiseParams in tinympc_rollout.h):
// the same text compiled with PLANT_NOISY. The step reads the TRUE state (px while measurement noise is on, else x0), adds the row's
// process noise behind the chain and the disturbance -- (acc + w) + (sw_r n), the product rounded first --, stores the true state where
// it read it, and where measurement noise is on writes x+ + (sv_r n) into x0: the measurement the next solve reads. The draw
// (rollout_normal, tinympc_rollout_noise.h) is a pure function of (seed, global instance, tick, row, stream): lane r of the wavefront
// form and row r of the workgroup form hand it the same counter. Lanes that are no state row draw nothing, a family that is off draws
// nothing. k_rollout_noise regenerates the terms of a range of ticks through the same function (tinympc_get_rollout_noise).
#include "tinympc_rollout.h"
#include "tinympc_rollout_noise.h"
#include "tinympc_sweep.h"

namespace tinympc {

constexpr int PLANT_WG_ROWS = 512;  // nx+nu of the largest system a handle takes (tinympc_setup_batch)

#define PLANT_NOISY 0
#define PLANT_SCORED 0
#include "tinympc_rollout_body.h"  // k_plant_step<W, KT>, k_plant_step_wg
#undef PLANT_SCORED

template <int W, int KT>
static hipError_t launch_plant_step_w(const PlantStepParams &p, hipStream_t stream) {
    const size_t blocks = ((size_t)p.batch * W + 255) / 256;
    hipLaunchKernelGGL((k_plant_step<W, KT>), dim3((unsigned)blocks), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_plant_step(const PlantStepParams &p, int W, int KT, hipStream_t stream) {
    if (p.batch < 1 || p.nx < 1 || p.nu < 1 || p.ticks < 1 || p.t < 0 || p.t >= p.ticks || !p.A || !p.B || !p.f || !p.x0 || !p.sol_u || !p.istats)
        return hipErrorInvalidValue;
    if (W > 64) {
        if (p.nx + p.nu > PLANT_WG_ROWS) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_plant_step_wg, dim3((unsigned)p.batch), dim3(256), 0, stream, p);
        return hipGetLastError();
    }
    if (p.nx + p.nu > KT) return hipErrorInvalidValue;
    if (W == 16 && KT == 8) return launch_plant_step_w<16, 8>(p, stream);
    if (W == 16 && KT == 12) return launch_plant_step_w<16, 12>(p, stream);
    if (W == 16 && KT == 16) return launch_plant_step_w<16, 16>(p, stream);
    if (W == 32 && KT == 32) return launch_plant_step_w<32, 32>(p, stream);
    if (W == 64 && KT == 64) return launch_plant_step_w<64, 64>(p, stream);
    return hipErrorInvalidValue;
}

#define PLANT_SCORED 1
#include "tinympc_rollout_body.h"  // k_plant_step_scored<W, KT>, k_plant_step_wg_scored
#undef PLANT_SCORED

template <int W, int KT>
static hipError_t launch_plant_step_scored_w(const PlantStepParams &p, const PlantMetricsParams &q, hipStream_t stream) {
    const size_t blocks = ((size_t)p.batch * W + 255) / 256;
    hipLaunchKernelGGL((k_plant_step_scored<W, KT>), dim3((unsigned)blocks), dim3(256), 0, stream, p, q);
    return hipGetLastError();
}

hipError_t launch_plant_step_scored(const PlantStepParams &p, const PlantMetricsParams &q, int W, int KT, hipStream_t stream) {
    if (p.batch < 1 || p.nx < 1 || p.nu < 1 || p.ticks < 1 || p.t < 0 || p.t >= p.ticks || !p.A || !p.B || !p.f || !p.x0 || !p.sol_u || !p.istats)
        return hipErrorInvalidValue;
    if (!q.rows || !q.qx || !q.ru || !q.xr || !q.ur || q.xr_T < 0 || q.ur_T < 0 || ((q.xr_T > 0 || q.ur_T > 0) && !q.steps) ||
        (q.xlo && !q.xhi) || (q.ulo && !q.uhi))
        return hipErrorInvalidValue;
    if (W > 64) {
        if (p.nx + p.nu > PLANT_WG_ROWS) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_plant_step_wg_scored, dim3((unsigned)p.batch), dim3(256), 0, stream, p, q);
        return hipGetLastError();
    }
    if (p.nx + p.nu > KT) return hipErrorInvalidValue;
    if (W == 16 && KT == 8) return launch_plant_step_scored_w<16, 8>(p, q, stream);
    if (W == 16 && KT == 12) return launch_plant_step_scored_w<16, 12>(p, q, stream);
    if (W == 16 && KT == 16) return launch_plant_step_scored_w<16, 16>(p, q, stream);
    if (W == 32 && KT == 32) return launch_plant_step_scored_w<32, 32>(p, q, stream);
    if (W == 64 && KT == 64) return launch_plant_step_scored_w<64, 64>(p, q, stream);
    return hipErrorInvalidValue;
}

#undef PLANT_NOISY
#define PLANT_NOISY 1
#define PLANT_SCORED 0
#include "tinympc_rollout_body.h"  // k_plant_step_noisy<W, KT>, k_plant_step_wg_noisy
#undef PLANT_SCORED
#define PLANT_SCORED 1
#include "tinympc_rollout_body.h"  // k_plant_step_scored_noisy<W, KT>, k_plant_step_wg_scored_noisy
#undef PLANT_SCORED
#undef PLANT_NOISY

template <int W, int KT>
static hipError_t launch_plant_step_noisy_w(const PlantStepParams &p, const PlantMetricsParams *q, const PlantNoiseParams &n, hipStream_t stream) {
    const size_t blocks = ((size_t)p.batch * W + 255) / 256;
    if (q) hipLaunchKernelGGL((k_plant_step_scored_noisy<W, KT>), dim3((unsigned)blocks), dim3(256), 0, stream, p, *q, n);
    else hipLaunchKernelGGL((k_plant_step_noisy<W, KT>), dim3((unsigned)blocks), dim3(256), 0, stream, p, n);
    return hipGetLastError();
}

hipError_t launch_plant_step_noisy(const PlantStepParams &p, const PlantMetricsParams *q, const PlantNoiseParams &n, int W, int KT, hipStream_t stream) {
    if (p.batch < 1 || p.nx < 1 || p.nu < 1 || p.ticks < 1 || p.t < 0 || p.t >= p.ticks || !p.A || !p.B || !p.f || !p.x0 || !p.sol_u || !p.istats)
        return hipErrorInvalidValue;
    if (q && (!q->rows || !q->qx || !q->ru || !q->xr || !q->ur || q->xr_T < 0 || q->ur_T < 0 || ((q->xr_T > 0 || q->ur_T > 0) && !q->steps) ||
              (q->xlo && !q->xhi) || (q->ulo && !q->uhi)))
        return hipErrorInvalidValue;
    // (the true state lives beside x0 exactly while there is measurement noise; a global index is 32 bits of the counter)
    if ((!n.sw && !n.sv) || (n.sv != nullptr) != (n.px != nullptr) || n.first_instance + (unsigned long long)p.batch > (1ull << 32))
        return hipErrorInvalidValue;
    if (W > 64) {
        if (p.nx + p.nu > PLANT_WG_ROWS) return hipErrorInvalidValue;
        if (q) hipLaunchKernelGGL(k_plant_step_wg_scored_noisy, dim3((unsigned)p.batch), dim3(256), 0, stream, p, *q, n);
        else hipLaunchKernelGGL(k_plant_step_wg_noisy, dim3((unsigned)p.batch), dim3(256), 0, stream, p, n);
        return hipGetLastError();
    }
    if (p.nx + p.nu > KT) return hipErrorInvalidValue;
    if (W == 16 && KT == 8) return launch_plant_step_noisy_w<16, 8>(p, q, n, stream);
    if (W == 16 && KT == 12) return launch_plant_step_noisy_w<16, 12>(p, q, n, stream);
    if (W == 16 && KT == 16) return launch_plant_step_noisy_w<16, 16>(p, q, n, stream);
    if (W == 32 && KT == 32) return launch_plant_step_noisy_w<32, 32>(p, q, n, stream);
    if (W == 64 && KT == 64) return launch_plant_step_noisy_w<64, 64>(p, q, n, stream);
    return hipErrorInvalidValue;
}

// One thread per (instance, tick, row) of the disturbance's layout: the terms the noisy steps of these ticks add, by the steps' own draw.
__global__ void __launch_bounds__(256) k_rollout_noise(const PlantNoiseParams n, int nx, int batch, int ticks, double *w_out, double *v_out) {
#pragma clang fp contract(off)
    const size_t total = (size_t)batch * ticks * nx;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const unsigned r = (unsigned)(i % nx);
        const size_t bt = i / nx;
        const size_t b = bt / ticks;
        const unsigned tick = n.tick + (unsigned)(bt % ticks);
        const unsigned g = (unsigned)(n.first_instance + (unsigned long long)b);
        if (w_out) w_out[i] = n.sw ? n.sw[b * n.sw_stride + r] * rollout_normal(n.key0, n.key1, g, tick, r, 0u) : 0.0;
        if (v_out) v_out[i] = n.sv ? n.sv[b * n.sv_stride + r] * rollout_normal(n.key0, n.key1, g, tick, r, 1u) : 0.0;
    }
}
hipError_t launch_rollout_noise(const PlantNoiseParams &n, int nx, int batch, int ticks, double *w_out, double *v_out, hipStream_t stream) {
    if (nx < 1 || batch < 1 || ticks < 1 || n.first_instance + (unsigned long long)batch > (1ull << 32) ||
        (unsigned long long)n.tick + (unsigned long long)ticks > (1ull << 32))
        return hipErrorInvalidValue;
    if (!w_out && !v_out) return hipSuccess;
    const size_t blocks = ((size_t)batch * ticks * nx + 255) / 256;
    hipLaunchKernelGGL(k_rollout_noise, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, stream, n, nx, batch, ticks, w_out, v_out);
    return hipGetLastError();
}

__global__ void __launch_bounds__(256) k_check_finite(const double *v, size_t n, int *flag) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        if (!(fabs(v[i]) <= 1.79769313486231570815e308)) *flag = 1;  // (NaN and the infinities fail the test)
}
hipError_t launch_check_finite(const double *v, size_t n, int *flag, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_check_finite, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, stream, v, n, flag);
    return hipGetLastError();
}

}  // namespace tinympc
