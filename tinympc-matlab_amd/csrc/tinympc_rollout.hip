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
#include "tinympc_rollout.h"
#include "tinympc_sweep.h"

namespace tinympc {

template <int W, int KT>
__global__ void __launch_bounds__(256) k_plant_step(const PlantStepParams p) {
    const int nx = p.nx, nu = p.nu, nxu = nx + nu;
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    const long b = gid / W;
    const int r = (int)(gid % W);
    const bool live = b < p.batch;
    const bool xrow = live && r < nx, urow = live && r >= nx && r < nxu;
    double z = 0.0, c = 0.0, wd = 0.0;
    // Row r of A_p | B_p, zeros beyond nx+nu and in lanes that are no row. The loads are unconditional -- a lane that is no row reads
    // row 0 of instance 0 and drops it --, so all KT of them are in flight at once (the column tests are wave-uniform).
    double m[KT];
    {
        const size_t bl = xrow ? (size_t)b : 0;
        const int rl = xrow ? r : 0;
        const double *Ar = p.A + bl * p.A_stride + rl, *Br = p.B + bl * p.B_stride + rl;
#pragma unroll
        for (int k = 0; k < KT; ++k) {
            const bool in = k < nxu;
            const double *q = k < nx ? Ar + (size_t)k * nx : Br + (size_t)(in ? k - nx : 0) * nx;
            const double v = *q;
            m[k] = (in && xrow) ? v : 0.0;
        }
    }
    if (xrow) {
        z = p.x0[(size_t)b * nx + r];
        c = p.f[(size_t)b * p.f_stride + r];
        if (p.w) wd = p.w[((size_t)b * p.ticks + p.t) * nx + r];
        if (p.x_log) p.x_log[((size_t)b * (p.ticks + 1) + p.t) * nx + r] = z;
    } else if (urow) {
        z = p.sol_u[(size_t)b * p.u_stride + (r - nx)];
        if (p.u_log) p.u_log[((size_t)b * p.ticks + p.t) * nu + (r - nx)] = z;
    }
    if (live && r == 0) {
        if (p.iter_log) p.iter_log[(size_t)b * p.ticks + p.t] = p.istats[2 * (size_t)b];
        if (p.status_log) p.status_log[(size_t)b * p.ticks + p.t] = p.istats[2 * (size_t)b + 1];
    }
    // (every lane of the wavefront runs the chain: the DPP reads reach into lanes that store nothing)
    double acc = group_matvec<W, KT>(m, z, c);
    if (p.w) acc += wd;
    if (xrow) {
        p.x0[(size_t)b * nx + r] = acc;
        if (p.t == p.ticks - 1 && p.x_log) p.x_log[((size_t)b * (p.ticks + 1) + p.ticks) * nx + r] = acc;
    }
}

constexpr int PLANT_WG_ROWS = 512;  // nx+nu of the largest system a handle takes (tinympc_setup_batch)

__global__ void __launch_bounds__(256) k_plant_step_wg(const PlantStepParams p) {
    __shared__ double zs[PLANT_WG_ROWS];
    const int nx = p.nx, nu = p.nu, nxu = nx + nu;
    const size_t b = blockIdx.x;
    for (int i = threadIdx.x; i < nxu; i += 256) {
        if (i < nx) {
            const double v = p.x0[b * nx + i];
            zs[i] = v;
            if (p.x_log) p.x_log[(b * (p.ticks + 1) + p.t) * nx + i] = v;
        } else {
            const double v = p.sol_u[b * p.u_stride + (i - nx)];
            zs[i] = v;
            if (p.u_log) p.u_log[(b * p.ticks + p.t) * nu + (i - nx)] = v;
        }
    }
    if (threadIdx.x == 0) {
        if (p.iter_log) p.iter_log[b * p.ticks + p.t] = p.istats[2 * b];
        if (p.status_log) p.status_log[b * p.ticks + p.t] = p.istats[2 * b + 1];
    }
    __syncthreads();
    for (int r = threadIdx.x; r < nx; r += 256) {
        const double *Ar = p.A + b * p.A_stride + r, *Br = p.B + b * p.B_stride + r;
        double acc = p.f[b * p.f_stride + r];
        for (int k = 0; k < nx; ++k) acc = fma(Ar[(size_t)k * nx], zs[k], acc);
        for (int k = 0; k < nu; ++k) acc = fma(Br[(size_t)k * nx], zs[nx + k], acc);
        if (p.w) acc += p.w[(b * p.ticks + p.t) * nx + r];
        p.x0[b * nx + r] = acc;
        if (p.t == p.ticks - 1 && p.x_log) p.x_log[(b * (p.ticks + 1) + p.ticks) * nx + r] = acc;
    }
}

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
