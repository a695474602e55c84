// tinympc_rollout_body.h -- the two forms of k_plant_step, included by tinympc_rollout.hip once per variant (no include guard):
//   PLANT_SCORED 0   k_plant_step<W, KT>, k_plant_step_wg                     (const PlantStepParams p)
//   PLANT_SCORED 1   k_plant_step_scored<W, KT>, k_plant_step_wg_scored       (const PlantStepParams p, const PlantMetricsParams q)
// and, with PLANT_NOISY 1 beside either (the rollout noise: PlantNoiseParams n, tinympc_rollout.h; the draw: tinympc_rollout_noise.h),
//   PLANT_SCORED 0   k_plant_step_noisy<W, KT>, k_plant_step_wg_noisy                  (p, n)
//   PLANT_SCORED 1   k_plant_step_scored_noisy<W, KT>, k_plant_step_wg_scored_noisy    (p, q, n)
// One text for all: the plain kernels are what the preprocessor leaves without the scored and the noisy blocks, token for token what they
// were before the variants existed (a shared template body with a compile-time flag renamed scalar registers in the plain kernels; this
// does not). Where a noisy block REPLACES a line, the line stands unchanged behind its #else.
#if PLANT_SCORED && PLANT_NOISY
#define PLANT_KERNEL(name) name##_scored_noisy
#define PLANT_KERNEL_ARGS const PlantStepParams p, const PlantMetricsParams q, const PlantNoiseParams n
#elif PLANT_NOISY
#define PLANT_KERNEL(name) name##_noisy
#define PLANT_KERNEL_ARGS const PlantStepParams p, const PlantNoiseParams n
#elif PLANT_SCORED
#define PLANT_KERNEL(name) name##_scored
#define PLANT_KERNEL_ARGS const PlantStepParams p, const PlantMetricsParams q
#else
#define PLANT_KERNEL(name) name
#define PLANT_KERNEL_ARGS const PlantStepParams p
#endif

template <int W, int KT>
__global__ void __launch_bounds__(256) PLANT_KERNEL(k_plant_step)(PLANT_KERNEL_ARGS) {
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
#if PLANT_NOISY
    double sw = 0.0, sv = 0.0;  // the row's noise scales (a family that is off, and a lane that is no state row: nothing drawn)
#endif
    if (xrow) {
#if PLANT_NOISY
        z = (n.px ? n.px : p.x0)[(size_t)b * nx + r];  // the true state
        if (n.sw) sw = n.sw[(size_t)b * n.sw_stride + r];
        if (n.sv) sv = n.sv[(size_t)b * n.sv_stride + r];
#else
        z = p.x0[(size_t)b * nx + r];
#endif
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
#if PLANT_NOISY
    if (xrow) {
#pragma clang fp contract(off)
        const unsigned g = (unsigned)(n.first_instance + (unsigned long long)b);
        if (n.sw) acc = acc + sw * rollout_normal(n.key0, n.key1, g, n.tick, (unsigned)r, 0u);
        (n.px ? n.px : p.x0)[(size_t)b * nx + r] = acc;
        if (p.t == p.ticks - 1 && p.x_log) p.x_log[((size_t)b * (p.ticks + 1) + p.ticks) * nx + r] = acc;
        if (n.sv) p.x0[(size_t)b * nx + r] = acc + sv * rollout_normal(n.key0, n.key1, g, n.tick, (unsigned)r, 1u);  // what the next solve reads
    }
#else
    if (xrow) {
        p.x0[(size_t)b * nx + r] = acc;
        if (p.t == p.ticks - 1 && p.x_log) p.x_log[((size_t)b * (p.ticks + 1) + p.ticks) * nx + r] = acc;
    }
#endif
#if PLANT_SCORED
    {
#pragma clang fp contract(off)
        // the row's term of the cost, its breach of the bounds and (state rows) |e|; zeros in lanes that are no row
        double term = 0.0, ea = 0.0, vx = 0.0, vu = 0.0;
        if (xrow) {
            size_t col = 0;
            if (q.xr_T) { const int st = q.steps[b]; col = (size_t)(st < q.xr_T ? st : q.xr_T - 1); }
            const double e = z - q.xr[(size_t)b * q.xr_stride + col * nx + r];
            term = q.qx[r] * (e * e);
            ea = fabs(e);
            if (q.xlo) vx = fmax(0.0, fmax(q.xlo[(size_t)b * q.xb_stride + r] - z, z - q.xhi[(size_t)b * q.xb_stride + r]));
        } else if (urow) {
            const int j = r - nx;
            size_t col = 0;
            if (q.ur_T) { const int st = q.steps[b]; col = (size_t)(st < q.ur_T ? st : q.ur_T - 1); }
            const double d = z - q.ur[(size_t)b * q.ur_stride + col * nu + j];
            term = q.ru[j] * (d * d);
            if (q.ulo) vu = fmax(0.0, fmax(q.ulo[(size_t)b * q.ub_stride + j] - z, z - q.uhi[(size_t)b * q.ub_stride + j]));
        }
        const bool slot = live && r < 8;  // lane r of the instance owns slot r of its row
        double mine = 0.0, s0 = 0.0;
        int it = 0, status = 1;
        if (slot) {
            mine = q.rows[(size_t)b * 8 + r];
            s0 = q.rows[(size_t)b * 8];
            it = p.istats[2 * (size_t)b];
            status = p.istats[2 * (size_t)b + 1];
        }
        // the cost: the plant's chain over a matrix of ones, from the stored cost in lane 1 -- fma(1, term_k, acc), k ascending
        double ones[KT];
#pragma unroll
        for (int k = 0; k < KT; ++k) ones[k] = 1.0;
        const double cost = group_matvec<W, KT>(ones, term, r == 1 ? mine : 0.0);
        const double mvx = group_max<W>(vx), mvu = group_max<W>(vu), mea = group_max<W>(ea);
        const double out = r == 0   ? mine + 1.0
                           : r == 1 ? cost
                           : r == 2 ? fmax(mine, mvx)
                           : r == 3 ? fmax(mine, mvu)
                           : r == 4 ? mine + (double)it
                           : r == 5 ? fmax(mine, (double)it)
                           : r == 6 ? mine + (status != 1 ? 1.0 : 0.0)
                                    : ((q.settle_tol > 0.0 && mea > q.settle_tol) ? s0 + 1.0 : mine);
        if (slot) q.rows[(size_t)b * 8 + r] = out;
    }
#endif
}

__global__ void __launch_bounds__(256) PLANT_KERNEL(k_plant_step_wg)(PLANT_KERNEL_ARGS) {
    __shared__ double zs[PLANT_WG_ROWS];
#if PLANT_SCORED
    __shared__ double ms[3 * PLANT_WG_ROWS];  // the rows' terms | breaches | |e|
#endif
    const int nx = p.nx, nu = p.nu, nxu = nx + nu;
    const size_t b = blockIdx.x;
    for (int i = threadIdx.x; i < nxu; i += 256) {
        if (i < nx) {
#if PLANT_NOISY
            const double v = (n.px ? n.px : p.x0)[b * nx + i];  // the true state
#else
            const double v = p.x0[b * nx + i];
#endif
            zs[i] = v;
            if (p.x_log) p.x_log[(b * (p.ticks + 1) + p.t) * nx + i] = v;
#if PLANT_SCORED
            {
#pragma clang fp contract(off)
                size_t col = 0;
                if (q.xr_T) { const int st = q.steps[b]; col = (size_t)(st < q.xr_T ? st : q.xr_T - 1); }
                const double e = v - q.xr[b * q.xr_stride + col * nx + i];
                ms[i] = q.qx[i] * (e * e);
                ms[PLANT_WG_ROWS + i] = q.xlo ? fmax(0.0, fmax(q.xlo[b * q.xb_stride + i] - v, v - q.xhi[b * q.xb_stride + i])) : 0.0;
                ms[2 * PLANT_WG_ROWS + i] = fabs(e);
            }
#endif
        } else {
            const double v = p.sol_u[b * p.u_stride + (i - nx)];
            zs[i] = v;
            if (p.u_log) p.u_log[(b * p.ticks + p.t) * nu + (i - nx)] = v;
#if PLANT_SCORED
            {
#pragma clang fp contract(off)
                const int j = i - nx;
                size_t col = 0;
                if (q.ur_T) { const int st = q.steps[b]; col = (size_t)(st < q.ur_T ? st : q.ur_T - 1); }
                const double d = v - q.ur[b * q.ur_stride + col * nu + j];
                ms[i] = q.ru[j] * (d * d);
                ms[PLANT_WG_ROWS + i] = q.ulo ? fmax(0.0, fmax(q.ulo[b * q.ub_stride + j] - v, v - q.uhi[b * q.ub_stride + j])) : 0.0;
            }
#endif
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
#if PLANT_NOISY
        {
#pragma clang fp contract(off)
            const unsigned g = (unsigned)(n.first_instance + (unsigned long long)b);
            if (n.sw) acc = acc + n.sw[b * n.sw_stride + r] * rollout_normal(n.key0, n.key1, g, n.tick, (unsigned)r, 0u);
            (n.px ? n.px : p.x0)[b * nx + r] = acc;
            if (p.t == p.ticks - 1 && p.x_log) p.x_log[(b * (p.ticks + 1) + p.ticks) * nx + r] = acc;
            if (n.sv) p.x0[b * nx + r] = acc + n.sv[b * n.sv_stride + r] * rollout_normal(n.key0, n.key1, g, n.tick, (unsigned)r, 1u);
        }
#else
        p.x0[b * nx + r] = acc;
        if (p.t == p.ticks - 1 && p.x_log) p.x_log[(b * (p.ticks + 1) + p.ticks) * nx + r] = acc;
#endif
    }
#if PLANT_SCORED
    if (threadIdx.x == 0) {  // the terms are behind the barrier above: the same chain, rows ascending, and the maxima
#pragma clang fp contract(off)
        double *row = q.rows + b * 8;
        double cost = row[1], mvx = 0.0, mvu = 0.0, mea = 0.0;
        for (int i = 0; i < nxu; ++i) cost = cost + ms[i];
        for (int i = 0; i < nx; ++i) {
            mvx = fmax(mvx, ms[PLANT_WG_ROWS + i]);
            mea = fmax(mea, ms[2 * PLANT_WG_ROWS + i]);
        }
        for (int i = nx; i < nxu; ++i) mvu = fmax(mvu, ms[PLANT_WG_ROWS + i]);
        const int it = p.istats[2 * b], status = p.istats[2 * b + 1];
        const double s1 = row[0] + 1.0;
        row[0] = s1;
        row[1] = cost;
        row[2] = fmax(row[2], mvx);
        row[3] = fmax(row[3], mvu);
        row[4] = row[4] + (double)it;
        row[5] = fmax(row[5], (double)it);
        row[6] = row[6] + (status != 1 ? 1.0 : 0.0);
        if (q.settle_tol > 0.0 && mea > q.settle_tol) row[7] = s1;
    }
#endif
}

#undef PLANT_KERNEL
#undef PLANT_KERNEL_ARGS
