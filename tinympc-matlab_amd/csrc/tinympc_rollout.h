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

// W, KT: the handle's lanes per instance and padded operand length (choose_geometry); W > 64 (layout M's systems): the workgroup form.
hipError_t launch_plant_step(const PlantStepParams &p, int W, int KT, hipStream_t stream);
// *flag = 1 where v holds a value that is not finite (device input of tinympc_set_plant_batch_device)
hipError_t launch_check_finite(const double *v, size_t n, int *flag, hipStream_t stream);

}  // namespace tinympc
