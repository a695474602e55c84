// tinympc_rollout.h -- the plant step behind a tick's solve (tinympc_rollout.hip): what tinympc_rollout_batch, its _device form and
// tinympc_plant_step_batch queue on the handle's stream.
#pragma once
#include <hip/hip_runtime.h>

namespace tinympc {

// One tick of every instance b of the batch:  x = x0[b], u = sol_u[b][:, 0], (it, status) = istats[b];
//   x_log[b][:, t] = x, u_log[b][:, t] = u, iter_log[b][t] = it, status_log[b][t] = status   (each where its pointer is set),
//   x+ = A_p x + B_p u + f_p + w[b][:, t]  ->  x0[b]  (and x_log[b][:, ticks] on the last tick).
// The plant operands are one pointer each with an instance stride in doubles (0: one shared plant), column-major as the handle keeps
// its model. The logs are instance-major, the layout of the reference tracks: x_log nx x (ticks+1) x batch, u_log nu x ticks x batch,
// iter_log / status_log ticks x batch, w nx x ticks x batch.
struct PlantStepParams {
    int nx, nu, batch;
    int t, ticks;              // this tick and the length of the rollout (a single plant step: t = 0, ticks = 1)
    size_t u_stride;           // doubles between two instances' controls in sol_u: nu x (N-1)
    const double *A, *B, *f;   // the plant; f is never NULL (a plant without an affine term keeps zeros there)
    size_t A_stride, B_stride, f_stride;
    const double *w;           // the disturbance, or NULL
    double *x0;                // [batch][nx], advanced in place
    const double *sol_u;
    const int *istats;         // [batch][2]: iterations, status
    double *x_log, *u_log;
    int *iter_log, *status_log;
};

// The rollout metrics (tinympc_set_rollout_metrics): one row of 8 doubles per instance, accumulated by the scored variant of the step
// from what the step holds in registers anyway. With x, u as above, e = x - xr, d = u - ur (xr, ur: the reference the solve tracked at
// knot 0), lo / hi its bounds at knot 0 and t the row's own step count:
//   [0] steps                      += 1
//   [1] cost                       one chain from the stored value: + qx_i (e_i e_i), state rows ascending, then + ru_j (d_j d_j), input
//                                  rows ascending; every product rounded once, nothing contracted into the add
//   [2] worst state-bound breach   max(., max_i max(0, lo_i - x_i, x_i - hi_i))    (xlo NULL: the family is off, 0)
//   [3] worst input-bound breach   the same for u                                    (ulo NULL: 0)
//   [4] iterations                 += istats[2b]
//   [5] most iterations of a step  max(., istats[2b])
//   [6] unconverged steps          += (istats[2b+1] != 1: anything but TINYMPC_STATUS_SOLVED -- a tick that ran out of iterations reports 11)
//   [7] settle step                t + 1 of this step where max_i |e_i| > settle_tol (and settle_tol > 0), else kept
// A reference / bound operand is a pointer, an instance stride in doubles (0: shared) and a column: min(steps[b], T - 1) where T > 0 (a
// half in track mode, read before the auto-advance), else 0. Columns are nx (nu) doubles apart.
struct PlantMetricsParams {
    double *rows;                      // [batch][8]
    const double *qx, *ru;             // the weights, nx | nu, shared by the batch
    double settle_tol;
    const double *xr, *ur;
    size_t xr_stride, ur_stride;
    int xr_T, ur_T;
    const int *steps;                  // the tracks' steps (read where xr_T or ur_T > 0)
    const double *xlo, *xhi, *ulo, *uhi;
    size_t xb_stride, ub_stride;
};

// The rollout noise (tinympc_set_rollout_noise): the noisy variants of the step draw it on the device (rollout_normal,
// tinympc_rollout_noise.h -- the draw n(g, tick, r, stream) is defined there). With x the TRUE state and acc the chain of the plain step
// (f_p, A_p's columns, B_p's columns; + w[b][:, t] where there is a disturbance):
//   x     = px ? px[b] : x0[b]                               x_log[b][:, t] = x; the scored block scores this x
//   acc   = acc + (sw_r * n(g, tick, r, 0))   where sw       the product rounded, then the add
//   x+    = acc  ->  px ? px[b] : x0[b]                      (and x_log[b][:, ticks] on the last tick)
//   x0[b][r] = x+ + (sv_r * n(g, tick, r, 1)) where sv       the measurement the NEXT solve reads
// g = first_instance + b. A scale vector is a pointer and an instance stride in doubles (0: one vector shared by the batch, nx: one per
// instance); NULL: that family is off and nothing is drawn for it. px ([batch][nx]) is set exactly while sv is.
struct PlantNoiseParams {
    unsigned key0, key1;               // seed & 0xffffffff, seed >> 32
    unsigned tick;                     // the handle's noise tick of this step
    unsigned long long first_instance;
    const double *sw, *sv;
    size_t sw_stride, sv_stride;
    double *px;
};

// W, KT: the handle's lanes per instance and padded operand length (choose_geometry); W > 64 (layout M's systems): the workgroup form.
hipError_t launch_plant_step(const PlantStepParams &p, int W, int KT, hipStream_t stream);
// ... and its scored variant: the same step (the same bits in x0 and the logs), and every instance's metrics row moves on
hipError_t launch_plant_step_scored(const PlantStepParams &p, const PlantMetricsParams &q, int W, int KT, hipStream_t stream);
// ... and the noisy variants of both (q NULL: not scored)
hipError_t launch_plant_step_noisy(const PlantStepParams &p, const PlantMetricsParams *q, const PlantNoiseParams &n, int W, int KT, hipStream_t stream);
// What the noisy steps of ticks n.tick .. n.tick + ticks - 1 add, regenerated: w_out = sw_r * n(g, tick, r, 0), v_out = sv_r * n(g, tick, r, 1),
// each nx x ticks x batch in the disturbance's layout (either may be NULL; a family that is off yields zeros)
hipError_t launch_rollout_noise(const PlantNoiseParams &n, int nx, int batch, int ticks, double *w_out, double *v_out, hipStream_t stream);
// *flag = 1 where v holds a value that is not finite (device input of tinympc_set_plant_batch_device)
hipError_t launch_check_finite(const double *v, size_t n, int *flag, hipStream_t stream);

}  // namespace tinympc
