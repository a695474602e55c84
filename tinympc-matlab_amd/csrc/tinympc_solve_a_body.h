// tinympc_solve_a_body.h -- the body of layout A's three solve kernels (k_admm_solve, k_admm_solve_fam, k_admm_solve_adapt;
// tinympc_solve_a.h; and k_admm_solve_iref, k_admm_solve_ibnd, k_admm_solve_imod, k_admm_solve_ifam, k_admm_solve_ifamk). Included INSIDE each kernel, with the kernel's template parameters W, KT,
// TLDS, GMEM, its parameter p and the variant E (SolveExt) in scope; the families', adaptive rho's and per-instance references' and
// bounds' additions are compiled only into their variant.
// No include guard: it is meant to be included once per kernel.
    // per-instance linear rows (with the per-instance rows of both kinds): the families' variant whose linear rows a_k | b_k | ||a_k||^2 are
    // this lane's INSTANCE's, from p.ilin, [group][3 nl][64] -- one 512-byte line per row vector and wavefront -- instead of the shared
    // description's; and whose cone SLOPES are the instance's too (tinympc_set_cone_slopes_batch), one vector per round in front of the
    // group's rows. The cones' structure -- roles, last rows, round masks --, the enable flags and everything else as in the families' variant
    // per-instance linear rows PER KNOT: that variant with one difference -- the store holds a slot of 3 nl row vectors for every step of the
    // forward sweep (SolveParams::ilin_knots = N of them per group, slot 0 = knot 0 on the state lanes, slot i+1 = what step i finishes: the
    // sweep's own skew, k_build_inst_lin_knots), the third vector already 1 / ||a_k||^2, and `families` takes the slot. The registers that
    // hold the constant rows for the whole solve hold the first KNOT_REG_ROWS rows of the step's slot and of the next step's, fetched a step ahead
    constexpr bool IFAMK = E == SolveExt::InstFamiliesKnots;
    constexpr bool IFAM = E == SolveExt::InstFamilies || IFAMK;
    constexpr bool FAM = E == SolveExt::Families || IFAM, ADAPT = E == SolveExt::Adaptive;
    // per-instance references: this instance's linref rows and pNref from p.iref_lr / iref_pn (HBM / L2, the lane's own 512-byte line
    // per knot) instead of the shared tables; everything else as on the box path
    // per-instance bounds (with the per-instance references' rows): this instance's clamp rows from p.ibnd, streamed like the linref rows
    // per-instance models (with the per-instance rows of both kinds): this lane's operator rows and constants from its INSTANCE's block
    // of p.ops, [batch][ops_doubles(W, KT)] -- loads at the start of the solve only; the sweeps are InstBounds' sweeps
    constexpr bool IMOD = E == SolveExt::InstModels;
    constexpr bool IBND = E == SolveExt::InstBounds || IMOD || IFAM;
    constexpr bool IREF = E == SolveExt::InstRefs || IBND;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    refresh_reference_tables(p, W, KT);  // references handed over in pinned host memory (single-instance handles; adaptive rho: never)
    constexpr int IPW = 64 / W;
    const int lane = threadIdx.x;
    const int j = lane / W, r = lane % W;
    const int nx = p.nx, nu = p.nu, N = p.N, nxu = nx + nu;
    const long grp = blockIdx.x;
    const long inst = grp * IPW + j;
    const bool is_x = r < nx;
    const bool is_u = (r >= nx) && (r < nxu);
    const bool inst_ok = inst < p.batch;
    const bool row_ok = inst_ok && (r < nxu);
    const int dstride = IPW * nu;
    const int dsize = (N - 1) * dstride;
    const int VOFF = (N + 2) * 64;             // sV[k] - sG[k]
    const int TOFF = (int)table_rows(N) * W;   // hi[k] - lo[k]
    const int ldummy = (N + 1) * 64 + lane;    // this lane's dummy slot (LDS row N+1)
    const int gdummy = N * 64 + lane;          // same in the HBM layout (row N)

    double *sG = GMEM ? (p.scratch + (size_t)blockIdx.x * p.scratch_stride) : smem;
    double *sV = sG + VOFF;
    double *sD = sV + VOFF;
    double *sT = sD + ((dsize + 64 + 1) & ~1);
    const double *tab = TLDS ? sT : p.tables;
    const double *t_lo = tab, *t_lr = tab + 2 * TOFF;

    double *gG = p.G + (size_t)grp * (N + 1) * 64;
    const size_t vbase = ((size_t)grp * v_rows(N) + V_PAD) * 64;  // knot 0 in the padded HBM layout
    double *gV = p.V + vbase;
    double *gGC = p.GC + vbase, *gGL = p.GL + vbase, *gLX = p.LX + vbase;  // (families)
    double *gD = p.D + (size_t)grp * dsize;

    // ---- one coalesced pass HBM -> LDS (512-byte lines); knot k lands in LDS row k+1
    for (int kn = 0; kn < N; ++kn) {
        sG[(kn + 1) * 64 + lane] = gG[kn * 64 + lane];
        sV[(kn + 1) * 64 + lane] = gV[kn * 64 + lane];
    }
    sG[lane] = 0.0;
    sV[lane] = 0.0;
    sG[ldummy] = 0.0;
    sV[ldummy] = 0.0;
    for (int i = lane; i < dsize; i += 64) sD[i] = gD[i];
    sD[dsize + lane] = 0.0;
    if (TLDS) {
        const int tn = (int)tables_doubles(W, N);
        for (int i = lane; i < tn; i += 64) sT[i] = p.tables[i];
    }

    // ---- per-lane operator rows and constants (registers for the whole solve)
    // Families, RED (wide systems, 32 / 64 lanes per instance): the cross-row quantities come from group REDUCTIONS instead of
    // mat-vecs with 0/1 mask rows. Three mask rows of KT doubles per lane next to the two operator rows are 640 VGPRs at 64 lanes:
    // the kernel lived in scratch (nx=48, nu=16 with one cone and two linear rows: 2.0 M iterations/s against 131 M on the box
    // path). What the masks encode is small: per round a lane's cone is known by its LAST row (the t entry, Ct's one column), its
    // role says whether it belongs to the tail; a cone's ||w||^2 is one group sum over its tail rows, t one lane read, a linear
    // row's a'x and a'u two group sums.
    constexpr bool RED = W > 16;
    // Adaptive rho, 64 lanes per instance: three operator rows of 64 doubles are 384 VGPRs and, with the adaptation's Pinf row,
    // more than a wavefront has -- the kernel spilled 200 of them. A sweep needs ONE operator (Mf forward, Mb backward; [A'; B']
    // only in the sweeps that adapt), so RELOAD keeps one row array and rebuilds it from L2 at the start of each sweep (layout D
    // does the same from LDS); the narrower forms keep all three resident.
    constexpr bool RELOAD = ADAPT && W == 64;
    double mf[KT], mb_store[RELOAD ? 1 : KT], mt[KT], cn[RED ? 1 : KT], ct[RED ? 1 : KT], ty[RED ? 1 : KT];
    double (&mb)[KT] = *reinterpret_cast<double (*)[KT]>(RELOAD ? &mf[0] : &mb_store[0]);  // (RELOAD: the one array, Mb during the backward sweep)
    const size_t M = (size_t)W * KT;
    const double *ops = p.ops;
    if constexpr (IMOD) ops += (size_t)(inst_ok ? inst : 0) * ops_doubles(W, KT);  // (lanes beyond the batch: instance 0's block)
    const double *Mf0 = ops + (size_t)r * KT, *Mb0 = ops + M + (size_t)r * KT;
    if constexpr (!ADAPT) {
        const double *Cn = p.fam + 4 * W + (size_t)r * KT, *Ct = Cn + M, *Ty = Ct + M;
#pragma unroll
        for (int k = 0; k < KT; ++k) {
            mf[k] = Mf0[k];
            mb[k] = Mb0[k];
            if constexpr (FAM && !RED) { cn[k] = Cn[k]; ct[k] = Ct[k]; ty[k] = Ty[k]; }
        }
    }
    // adaptive rho: derivative rows of the two sweep operators, [A'; B'] rows for the dual residual, Pinf rows (k_build_adapt)
    const double *Mt = p.adapt + (size_t)r * KT, *Pi = p.adapt + M + (size_t)r * KT, *dPi = p.adapt + 2 * M + (size_t)r * KT;
    const double *dMf = p.adapt + 3 * M + (size_t)r * KT, *dMb = p.adapt + 4 * M + (size_t)r * KT;
    auto load_forward = [&](double delta) {
#pragma unroll
        for (int k = 0; k < KT; ++k) mf[k] = fma(delta, dMf[k], Mf0[k]);
    };
    auto load_backward = [&](double delta) {
#pragma unroll
        for (int k = 0; k < KT; ++k) mb[k] = fma(delta, dMb[k], Mb0[k]);
    };
    auto load_operators = [&](double delta) {
        if constexpr (!RELOAD) {
            load_forward(delta);
            load_backward(delta);
        }
    };

    // Families, RED: per round q -- this lane's role / slope / last row of its cone (-1: in no cone of the round), and the set of
    // last rows (= of cones) of the round as a wave-uniform bit mask of group-relative lane numbers
    int r_role[MAX_ROUNDS], r_head[MAX_ROUNDS];
    double r_mu[MAX_ROUNDS], r_imu[MAX_ROUNDS];
    unsigned long long r_cones[MAX_ROUNDS];
    if constexpr (FAM && RED) {
        const int nrounds = (int)p.fam[fam_nround_offset(W, KT)];
#pragma unroll
        for (int q = 0; q < MAX_ROUNDS; ++q) {
            r_role[q] = 0; r_head[q] = -1; r_mu[q] = 0.0; r_imu[q] = 0.0; r_cones[q] = 0ull;
            if (q < nrounds) {  // (uniform)
                const double *rd = q == 0 ? p.fam : p.fam + fam_round_offset(W, KT, q);
                const double *ctq = q == 0 ? p.fam + 4 * W + M : rd + 2 * W + M;
                r_role[q] = (int)rd[r];
                if constexpr (IFAMK) r_mu[q] = p.ilin[(size_t)grp * inst_fam_block_doubles(p.ilin_nl, p.ilin_knots) + (size_t)q * 64 + lane];
                else r_mu[q] = IFAM ? p.ilin[(size_t)grp * inst_fam_group_doubles(p.ilin_nl) + (size_t)q * 64 + lane] : rd[W + r];
                r_imu[q] = (r_mu[q] != 0.0) ? 1.0 / r_mu[q] : 0.0;
                for (int k = 0; k < nxu; ++k)
                    if (ctq[(size_t)r * KT + k] != 0.0) r_head[q] = k;
                const unsigned long long heads = __ballot(r_head[q] == r);
                r_cones[q] = (W == 64) ? heads : (heads & ((1ull << (W % 64)) - 1ull));  // (every instance of the wave has the same cones)
            }
        }
    }
    const int role = FAM ? (int)p.fam[r] : 0;
    const bool famc = FAM && p.fam[2 * W + r] != 0.0, faml = FAM && p.fam[3 * W + r] != 0.0;
    // (per-instance rows: this wavefront's block at ilin + grp inst_fam_group_doubles(nl) -- one slope vector per round, then row vector v
    // at + (INST_FAM_SLOPE_ROWS + v) 64 --, this lane's entry at + lane = j W + r; the shared description keeps its count in front of the
    // vectors: base LB, vector stride LW -- lin_rows[LB + v LW + r] serves both)
    constexpr int LW = IFAM ? 64 : W, LB = IFAM ? INST_FAM_SLOPE_ROWS * 64 : 1;
    const double *lin_shared = p.fam + 4 * W + 3 * M;
    const int nl = IFAM ? p.ilin_nl : FAM ? (int)lin_shared[0] : 0;
    const double *lin_rows = IFAMK ? p.ilin + ((size_t)grp * inst_fam_block_doubles(nl, p.ilin_knots) + j * W)
                             : IFAM ? p.ilin + ((size_t)grp * inst_fam_group_doubles(nl) + j * W) : lin_shared;
    // (per-instance slopes: round q's vector of this wavefront leads its block, at lin_rows + q 64 -- an address without the row count)
    const double mu = IFAM ? lin_rows[r] : FAM ? p.fam[W + r] : 0.0;
    const double inv_mu = (mu != 0.0) ? 1.0 / mu : 0.0;  // (mu = 0: row in no cone)
    // the first FAM_REG_ROWS rows' coefficients in registers; problems with more rows (an equality constraint of five rows is
    // ten) read the rest from the family buffer (L2) where they are used
    double ak[FAM_REG_ROWS], bk[FAM_REG_ROWS], ink[FAM_REG_ROWS];  // ink = 1 / ||a_k||^2
#pragma unroll
    for (int k = 0; k < (FAM && !RED && !IFAMK ? FAM_REG_ROWS : 0); ++k) {
        // (the per-instance store holds nl >= 1 rows, not the shared description's capacity: a register beyond nl repeats row 0, never used;
        // a handle without any linear row holds one absent row there, a = 0, b = +inf, norm 1)
        const int kr = IFAM ? (k < nl ? k : 0) : k;
        ak[k] = lin_rows[LB + (size_t)(3 * kr + 0) * LW + r];
        bk[k] = lin_rows[LB + (size_t)(3 * kr + 1) * LW + r];
        ink[k] = 1.0 / lin_rows[LB + (size_t)(3 * kr + 2) * LW + r];
    }
    // rows per knot: REGR rows of the step's slot and of the next step's in registers (the rest is read per use, as above), slot s of this
    // lane at lin_rows + LB + s kslot + r
    constexpr int REGR = IFAMK ? KNOT_REG_ROWS : FAM_REG_ROWS;
    constexpr int KR = IFAMK && !RED && REGR > 0 ? REGR : 1;
    const size_t kslot = IFAMK ? (size_t)3 * nl * 64 : 0;
    KnotRows<KR> KA{}, KB{};  // the step's slot and the next step's, in turns
    auto load_knot = [&](KnotRows<KR> &d, const double *kp) {
        if constexpr (IFAMK && !RED) {
#pragma unroll
            for (int k = 0; k < REGR; ++k) {  // (a register beyond nl is written too, so that none of them is carried from step to step)
                const bool has = k < nl;    // (uniform)
                d.a[k] = has ? kp[(size_t)(3 * k + 0) * 64] : 0.0;
                d.b[k] = has ? kp[(size_t)(3 * k + 1) * 64] : 0.0;
                d.in[k] = has ? kp[(size_t)(3 * k + 2) * 64] : 0.0;
            }
        }
    };
    // rounds of the cone list beyond the first (cones that share rows are projected one after another, as upstream does)
    const int nround = FAM ? (int)p.fam[fam_nround_offset(W, KT)] : 0;
    // wave-uniform switches: is either family in use at all?
    const bool any_cone = FAM && __ballot(famc) != 0ull, any_lin = FAM && __ballot(faml) != 0ull;

    const double cf = ops[(size_t)2 * W * KT + r];
    const double cb = ops[(size_t)2 * W * KT + W + r];
    double pnref = IREF ? p.iref_pn[(size_t)grp * 64 + lane] : p.tables[(size_t)3 * TOFF + r];
    double rho = p.rho;
    const double rho0 = p.rho, dgr = ADAPT ? ops[2 * M + 2 * W + r] : 0.0;  // Q + rho0 / R + rho0 diagonal of this row (tiny_api.cpp:90-91)
    const double pnref0 = pnref, dpnref = ADAPT ? p.adapt[5 * M + r] : 0.0;
    // per-instance models: the instance's own rho (tinympc_set_rho_batch; the handle's where the verb never named it), constant over the solve
    if constexpr (IMOD) rho = inst_ok ? p.rho_inst[inst] : rho0;
    if constexpr (ADAPT) {
        rho = inst_ok ? p.rho_inst[inst] : rho0;  // persists across solves like cache->rho
        pnref = fma(rho - rho0, dpnref, pnref0);
        load_operators(rho - rho0);
        if constexpr (!RELOAD) {
#pragma unroll
            for (int k = 0; k < KT; ++k) mt[k] = Mt[k];
        }
    }
    // per-instance references: the first four rows the backward sweep reads (knots N-2 .. N-5) stay in registers for the whole solve, so
    // that no sweep starts waiting for HBM; the ring below keeps the rest of the rows four knots ahead
    // (per-instance linear rows at 64 lanes per instance: with two operator rows of 64 doubles a wavefront has no registers left for the
    // twelve -- the kernel lived in scratch, 120 bytes --; there every sweep fetches its first four rows when it starts)
    constexpr bool TOP_PER_SWEEP = IFAM && W == 64;
    double lr_top[IREF ? 4 : 1];
    if constexpr (IREF && !TOP_PER_SWEEP) {
        const double *t = p.iref_lr + ((size_t)grp * table_rows(N) + (N - 1)) * 64 + lane;
#pragma unroll
        for (int k = 0; k < 4; ++k) lr_top[k] = t[-64 * k];
    }
    // per-instance bounds: knot 0's rows (the state lanes' x_0 clamp) and the first four rows the forward sweep reads stay in registers
    // for the whole solve; the ring in the sweep keeps the rest four knots ahead. hi rows lie bhi doubles behind the lo rows.
    const size_t bhi = IBND ? inst_bnd_hi_offset((int)p.groups, N) : 0;
    double blo0 = 0.0, bhi0 = 0.0, blo_top[IBND ? 4 : 1], bhi_top[IBND ? 4 : 1];
    if constexpr (IBND) {
        const double *t = p.ibnd + ((size_t)grp * table_rows(N) + 1) * 64 + lane;  // row 1 = knot 0
        blo0 = t[0];
        bhi0 = t[bhi];
        t += (is_x ? 1 : 0) * 64;  // (koff, below: the first row a state lane's sweep reads is knot 1's)
#pragma unroll
        for (int k = 0; k < (TOP_PER_SWEEP ? 0 : 4); ++k) {
            blo_top[k] = t[64 * k];
            bhi_top[k] = t[bhi + 64 * k];
        }
    }
    const double x0v = (inst_ok && is_x) ? p.x0[inst * nx + r] : 0.0;
    if (p.x0_mirror && inst_ok && is_x) p.x0_mirror[inst * nx + r] = x0v;  // zero-copy tick: x0 came from host memory
    const int dIdx = is_u ? (j * nu + (r - nx)) : 0;
    const int koff = is_x ? 1 : 0;  // at step i a state lane finishes knot i+1, an input lane knot i
    const int cterm = p.check_termination;
    __syncthreads();

    // Families: the two extra families for one (row, knot) element with rollout value `val`: returns the row's contribution to
    // the linear cost and the new duals.
    // (rows per knot: kreg holds the first REGR rows of the element's slot, krow points at the slot -- vector v of it at krow[v 64])
    auto families = [&](double val, double gc_old, double gl_old, double &gc_new, double &gl_new, const KnotRows<KR> &kreg, const double *krow) -> double {
        double lx = 0.0;
        gc_new = gc_old;
        gl_new = gl_old;
        if constexpr (RED) {
            if (any_cone) {
                const double sv = val + gc_old;  // vcnew = x + gc (all rows of an enabled side)
                double vc = sv;
#pragma unroll
                for (int q = 0; q < MAX_ROUNDS; ++q) {
                    if (q < nround) {  // (uniform)
                        double a2 = 0.0;
                        for (unsigned long long m = r_cones[q]; m != 0ull; m &= m - 1ull) {  // one cone of the round after the other (uniform)
                            const int hc = __builtin_ctzll(m);
                            const bool mine = r_head[q] == hc;
                            const double tail2 = group_sum<W>((mine && r_role[q] == 1) ? vc * vc : 0.0);  // ||w||^2 of that cone
                            a2 = mine ? tail2 : a2;
                        }
                        const double t = __shfl(vc, r_head[q] >= 0 ? r_head[q] : r, W);  // last entry of the row's cone
                        vc = soc_project_element(vc, a2, t, r_mu[q], r_imu[q], r_role[q]);
                    }
                }
                const double gcn = sv - vc;  // gc + x - vcnew
                if (famc) {
                    gc_new = gcn;
                    lx -= rho * (vc - gcn);
                }
            }
            if (any_lin) {
                const double s0 = val + gl_old;
                double sv = s0;
#pragma unroll 1
                for (int k = 0; k < nl; ++k) {  // (uniform trip count; the rows' coefficients from the family buffer in L2)
                    double a_k, b_k, in_k;
                    if constexpr (IFAMK) {  // (the knot's slot; its third vector holds the reciprocal)
                        a_k = krow[(size_t)(3 * k + 0) * 64]; b_k = krow[(size_t)(3 * k + 1) * 64];
                        in_k = krow[(size_t)(3 * k + 2) * 64];
                    } else {
                        a_k = lin_rows[LB + (size_t)(3 * k + 0) * LW + r]; b_k = lin_rows[LB + (size_t)(3 * k + 1) * LW + r];
                        in_k = 1.0 / lin_rows[LB + (size_t)(3 * k + 2) * LW + r];
                    }
                    const double prod = a_k * sv;
                    const double dx = group_sum<W>(is_x ? prod : 0.0), du = group_sum<W>(is_u ? prod : 0.0);  // a_k' x | a_k' u
                    sv = halfspace_project_element(sv, is_x ? dx : du, a_k, b_k, in_k);
                }
                const double gln = s0 - sv;
                if (faml) {
                    gl_new = gln;
                    lx -= rho * (sv - gln);
                }
            }
            return lx;
        } else {
        if (any_cone) {
            const double sv = val + gc_old;                              // vcnew = x + gc (all rows of an enabled side)
            const double a2 = group_matvec<W, KT>(cn, sv * sv, 0.0);     // ||w||^2 of the row's cone
            const double t = group_matvec<W, KT>(ct, sv, 0.0);           // last entry of the row's cone
            double vc = soc_project_element(sv, a2, t, mu, inv_mu, role);
#pragma unroll 1
            for (int q = 1; q < nround; ++q) {                           // (uniform trip count; the masks of round q from L2)
                const double *rd = p.fam + fam_round_offset(W, KT, q);
                const int role_q = (int)rd[r];
                const double mu_q = IFAM ? lin_rows[q * 64 + r] : rd[W + r];
                double cq[KT], tq[KT];
#pragma unroll
                for (int k = 0; k < KT; ++k) {
                    cq[k] = rd[2 * W + (size_t)r * KT + k];
                    tq[k] = rd[2 * W + M + (size_t)r * KT + k];
                }
                const double a2q = group_matvec<W, KT>(cq, vc * vc, 0.0);
                const double tq_ = group_matvec<W, KT>(tq, vc, 0.0);
                vc = soc_project_element(vc, a2q, tq_, mu_q, (mu_q != 0.0) ? 1.0 / mu_q : 0.0, role_q);
            }
            const double gcn = sv - vc;                                  // gc + x - vcnew
            if (famc) {
                gc_new = gcn;
                lx -= rho * (vc - gcn);
            }
        }
        if (any_lin) {
            const double s0 = val + gl_old;
            double sv = s0;
#pragma unroll
            for (int k = 0; k < REGR; ++k) {
                if (k < nl) {                                            // wave-uniform
                    double a_r, b_r, in_r;
                    if constexpr (IFAMK) { a_r = kreg.a[k]; b_r = kreg.b[k]; in_r = kreg.in[k]; }
                    else { a_r = ak[k]; b_r = bk[k]; in_r = ink[k]; }
                    const double dot = group_matvec<W, KT>(ty, a_r * sv, 0.0);
                    sv = halfspace_project_element(sv, dot, a_r, b_r, in_r);
                }
            }
#pragma unroll 1
            for (int k = REGR; k < nl; ++k) {                            // (uniform trip count)
                double a_k, b_k, in_k;
                if constexpr (IFAMK) {
                    a_k = krow[(size_t)(3 * k + 0) * 64]; b_k = krow[(size_t)(3 * k + 1) * 64];
                    in_k = krow[(size_t)(3 * k + 2) * 64];
                } else {
                    a_k = lin_rows[LB + (size_t)(3 * k + 0) * LW + r]; b_k = lin_rows[LB + (size_t)(3 * k + 1) * LW + r];
                    in_k = 1.0 / lin_rows[LB + (size_t)(3 * k + 2) * LW + r];
                }
                const double dot = group_matvec<W, KT>(ty, a_k * sv, 0.0);
                sv = halfspace_project_element(sv, dot, a_k, b_k, in_k);
            }
            const double gln = s0 - sv;
            if (faml) {
                gl_new = gln;
                lx -= rho * (sv - gln);
            }
        }
        return lx;
        }
    };

    bool active = inst_ok;
    int it_done = 0;
    int status = 11;  // TINY_UNSOLVED (admm.cpp:114)
    bool res_valid = false;
    double snap_pri = 0.0, snap_dua = 0.0;  // this lane's residual maxima at its instance's last termination check
    double snap_rho = rho;                  // ... and the rho of that check (adaptive rho: it can change after the last check)

    for (int it = 0; it < p.max_iter; ++it) {  // admm.cpp:129
        if (__ballot(active) == 0ull) break;
        const bool check = (cterm > 0) && (((it + 1) % cterm) == 0);  // admm.cpp:91 (iter already incremented, :143)
        const bool st = active && row_ok;
        double pri, dua;
        const bool adapt = ADAPT && (it > 0) && (it % 5 == 0);  // admm.cpp:155
        double a_pr = 0.0, a_pn = 0.0, a_dr = 0.0, a_dn = 0.0;  // adaptation: primal res / norm, dual res / norm
        double x_last = x0v, g_last = 0.0;

        if constexpr (RELOAD) {
            load_forward(rho - rho0);
            if (adapt) {  // (uniform)
#pragma unroll
                for (int k = 0; k < KT; ++k) mt[k] = Mt[k];
            }
        }

        // ---------------- forward sweep (F1) with the row-local phases S1+D1+R1 fused in.
        // The reference returns from a converged solve BEFORE v <- vnew (admm.cpp:181-197), so its
        // workspace keeps the previous iteration's v/z: on check iterations the old value is streamed to
        // HBM while it is still in a register; on convergence that copy is exactly the reference's v/z.
        {   // knot 0, state lanes only: x_0 is given (tiny_set_x0), no mat-vec
            const bool on = st && is_x;
            const double g = sG[64 + lane], vold = sV[64 + lane];
            const double s = x0v + g;
            const double snew = IBND ? fmin(bhi0, fmax(blo0, s)) : fmin(t_lo[TOFF + W + r], fmax(t_lo[W + r], s));
            pri = is_x ? fabs(x0v - snew) : 0.0;
            dua = is_x ? fabs(vold - snew) : 0.0;
            double gcn, gln, lx;
            const double *krow0 = nullptr;
            KnotRows<KR> K0{};
            if constexpr (IFAMK) {  // knot 0's slot for this call, and slot 1 for step 0 of the sweep behind it
                krow0 = lin_rows + LB + r;
                load_knot(K0, krow0);
                load_knot(KA, krow0 + kslot);
            }
            if constexpr (FAM) lx = families(x0v, gGC[lane], gGL[lane], gcn, gln, K0, krow0);
            if (check) gV[on ? lane : gdummy] = vold;
            sG[on ? 64 + lane : ldummy] = s - snew;
            sV[on ? 64 + lane : ldummy] = snew;
            if constexpr (FAM) {
                gGC[on ? lane : gdummy] = gcn;
                gGL[on ? lane : gdummy] = gln;
                gLX[on ? lane : gdummy] = lx;
            }
        }
        {
            const double *pg = sG + (1 + koff) * 64 + lane;  // this lane's operands of step 0
            constexpr int BRS = IBND ? 64 : W;  // clamp row stride
            const double *pt = IBND ? p.ibnd + ((size_t)grp * table_rows(N) + 1 + koff) * 64 + lane : t_lo + (1 + koff) * W + r;
            const double *pd = sD + dIdx;
            double *ps = sG + (st ? (1 + koff) * 64 + lane : ldummy);
            double *pgv = gV + (st ? koff * 64 + lane : gdummy);
            const int inc = st ? 64 : 0;
            double xcur = x0v;
            if constexpr (TOP_PER_SWEEP) {
#pragma unroll
                for (int k = 0; k < 4; ++k) { blo_top[k] = pt[64 * k]; bhi_top[k] = pt[bhi + 64 * k]; }
            }
            FwdOperands A{pg[0], pg[VOFF], IBND ? blo_top[0] : pt[0], IBND ? bhi_top[0] : pt[TOFF], pd[0]}, B;
            // per-instance rows come from HBM / L2, not LDS: three more rows of each in flight (reads past the last group's rows land in
            // the hi rows or in the padding behind them, INST_LR_PAD; never used)
            double l1 = 0.0, l2 = 0.0, l3 = 0.0, h1 = 0.0, h2 = 0.0, h3 = 0.0;
            if constexpr (IBND) { l1 = blo_top[1]; l2 = blo_top[2]; l3 = blo_top[3]; h1 = bhi_top[1]; h2 = bhi_top[2]; h3 = bhi_top[3]; }
            // families: the duals gc | gl read one step ahead, the new ones and lx written where pgv writes
            const double *pgc = gGC + koff * 64 + lane, *pgl = gGL + koff * 64 + lane;
            double *pwc = gGC + (pgv - gV), *pwl = gGL + (pgv - gV), *pwx = gLX + (pgv - gV);
            if constexpr (FAM) { A.gc = pgc[0]; A.gl = pgl[0]; }
            double gprev = 0.0;  // adaptive: g_i of the state rows; the x_0 column has no -g_0 term (y_vector starts at g_1)
            const double *pk = nullptr;  // rows per knot: the slot of the step (the slot behind the last step's is padding)
            if constexpr (IFAMK) pk = lin_rows + LB + kslot + r;
            auto fstep = [&](const FwdOperands &cur, FwdOperands &nxt, const KnotRows<KR> &kcur, KnotRows<KR> &knxt) {
                const double w = is_x ? xcur : cur.dv;
                pg += 64;  // operands of the next step, fetched while this step's mat-vec runs
                pt += BRS;
                pd += dstride;
                if constexpr (FAM) { pgc += 64; pgl += 64; }
                if constexpr (IBND) {
                    nxt.g = pg[0]; nxt.vold = pg[VOFF]; nxt.dv = pd[0];
                    nxt.lo = l1; l1 = l2; l2 = l3; l3 = pt[3 * BRS];
                    nxt.hi = h1; h1 = h2; h2 = h3; h3 = pt[bhi + 3 * BRS];
                } else {
                    nxt.g = pg[0]; nxt.vold = pg[VOFF]; nxt.lo = pt[0]; nxt.hi = pt[TOFF]; nxt.dv = pd[0];
                }
                if constexpr (FAM) { nxt.gc = pgc[0]; nxt.gl = pgl[0]; }
                const double *krow = nullptr;
                if constexpr (IFAMK) { krow = pk; pk += kslot; load_knot(knxt, pk); }
                const double out = group_matvec<W, KT>(mf, w, cf);  // state lanes: x_{i+1}; input lanes: u_i
                double gnew, snew;
                project_element(out, cur.g, cur.lo, cur.hi, cur.vold, gnew, snew, pri, dua);
                double gcn, gln, lx;
                if constexpr (FAM) lx = families(out, cur.gc, cur.gl, gcn, gln, kcur, krow);
                if (check) *pgv = cur.vold;
                ps[0] = gnew;
                ps[VOFF] = snew;
                if constexpr (FAM) { *pwc = gcn; *pwl = gln; *pwx = lx; }
                ps += inc;
                pgv += inc;
                if constexpr (FAM) { pwc += inc; pwl += inc; pwx += inc; }
                if constexpr (ADAPT) {
                    if (adapt) {
                        // state lanes: column x_i (xcur, gprev) and row vnew_{i+1} (snew); input lanes: column / row u_i
                        const double t = group_matvec<W, KT>(mt, is_x ? gnew : 0.0, 0.0);  // [A'; B'] g_{i+1}
                        const double dgx = dgr * (is_x ? xcur : out);                       // Q.*x_i | R.*u_i  (= P x and q entries)
                        const double aty = is_x ? (t - gprev) : (gnew + t);
                        a_dn = fmax(amax2(a_dn, dgx), fabs(aty));
                        a_dr = amax2(a_dr, 2.0 * dgx + aty);
                        a_pr = amax2(a_pr, is_x ? snew : (out - snew));
                        a_pn = fmax(amax2(a_pn, snew), is_x ? 0.0 : fabs(out));
                    }
                    gprev = gnew;
                }
                xcur = out;
            };
            if constexpr (ADAPT) {
                // rolled: unrolled by two, the step with the adaptation's residuals needs more registers -- 265 VGPRs in the
                // <16, 16> GMEM form, one wavefront per SIMD instead of two
                for (int i = 0; i < N - 1; ++i) {
                    fstep(A, B, KA, KB);
                    A = B;
                }
            } else {
                int i = 0;
                for (; i + 2 <= N - 1; i += 2) {
                    fstep(A, B, KA, KB);
                    fstep(B, A, KB, KA);
                }
                if (i < N - 1) fstep(A, B, KA, KB);
            }
            x_last = xcur;   // x_{N-1} on state lanes
            g_last = gprev;  // g_{N-1}
        }
        if (active) it_done = it + 1;  // admm.cpp:143

        // ---------------- adaptive rho (admm.cpp:147-174)
        const double rho_lin = rho, pnref_lin = pnref;  // what update_linear_cost used this iteration
        if (adapt) {
            // column block x_{N-1}: Pinf x + Q.*x - g_{N-1} with the CURRENT (adapted) Pinf (rho_benchmark.cpp:112)
            double pr[KT];
            const double delta = rho - rho0;
#pragma unroll
            for (int k = 0; k < KT; ++k) pr[k] = fma(delta, dPi[k], Pi[k]);
            const double px = group_matvec<W, KT>(pr, is_x ? x_last : 0.0, 0.0);
            if (is_x) {
                const double qv = dgr * x_last;
                a_dn = fmax(fmax(amax2(a_dn, px), fabs(qv)), fabs(g_last));
                a_dr = amax2(a_dr, px + qv - g_last);
            }
            const double pri_res = group_max<W>(a_pr), pri_norm = group_max<W>(a_pn);
            const double dual_res = group_max<W>(a_dr), dual_norm = group_max<W>(a_dn);
            const double eps = 1e-10;  // rho_benchmark.cpp:190-197
            const double normalized_pri = pri_res / (pri_norm + eps);
            const double normalized_dual = dual_res / (dual_norm + eps);
            const double ratio = normalized_pri / (normalized_dual + eps);
            double new_rho = rho * sqrt(ratio);
            if (p.rho_clip) new_rho = fmin(fmax(new_rho, p.rho_min), p.rho_max);
            if (active) {
                rho = new_rho;
                pnref = fma(rho - rho0, dpnref, pnref0);
            }
            load_operators(rho - rho0);  // rho is unchanged for instances that are no longer active
        }

        // ---------------- R1: termination test (admm.cpp:93-101), box family only (as upstream with the families)
        if (check) {
            // decided element-wise with one ballot (max_i a_i < tol iff every a_i < tol; rho > 0): see tinympc_solve_b.hip.
            // A NaN residual fails the test. Adaptive rho: the rho after the adaptation (cache->rho, admm.cpp:95-96).
            const bool below = (pri < p.abs_pri_tol) && (dua * rho < p.abs_dua_tol);
            constexpr unsigned long long ones = (W == 64) ? ~0ull : ((1ull << (W % 64)) - 1ull);
            const bool conv = ((__ballot(below) >> (j * W)) & ones) == ones;
            if (active) {
                snap_pri = pri;
                snap_dua = dua;
                if constexpr (ADAPT) snap_rho = rho;
                res_valid = true;
                if (conv) {
                    status = 1;  // TINY_SOLVED: stop this instance before the backward pass (admm.cpp:181-192)
                    active = false;
                }
            }
        }

        // ---------------- backward sweep (B1, admm.cpp:13-20); linear cost (L1, :77-82) recomputed from V,G
        // (adaptive rho: the linear cost with the rho / Pinf of update_linear_cost, the operators with the new Kinf)
        {
            if constexpr (RELOAD) load_backward(rho - rho0);
            const bool stb = active && row_ok && is_u;
            const double *pb = sG + N * 64 + lane;  // knot N-1
            double pcur = pnref_lin - rho_lin * (pb[VOFF] - pb[0]);  // p_{N-1}, admm.cpp:81-82 (state lanes)
            pb -= 64;                                                  // knot N-2
            constexpr int LRS = IREF ? 64 : W;  // linref row stride
            const double *pl = IREF ? p.iref_lr + ((size_t)grp * table_rows(N) + (N - 1)) * 64 + lane : t_lr + (N - 1) * W + r;
            double *pdst = sD + (stb ? (N - 2) * dstride + dIdx : dsize + lane);
            const int ddec = stb ? dstride : 0;
            if constexpr (TOP_PER_SWEEP) {
#pragma unroll
                for (int k = 0; k < 4; ++k) lr_top[k] = pl[-64 * k];
            }
            BwdOperands A{pb[0], pb[VOFF], IREF ? lr_top[0] : pl[0]}, B;
            // per-instance rows come from HBM / L2, not LDS: three more rows in flight (rows below row 0 are the previous group's or the
            // buffer's padding, INST_LR_PAD; never used)
            double q1 = 0.0, q2 = 0.0, q3 = 0.0;
            if constexpr (IREF) { q1 = lr_top[1]; q2 = lr_top[2]; q3 = lr_top[3]; }
            const double *px_ = gLX + (N - 1) * 64 + lane;  // families: lx, knot N-1 first
            if constexpr (FAM) {
                pcur += px_[0];  // p_{N-1} incl. the family terms
                px_ -= 64;
                A.lx = px_[0];
            }
            auto bstep = [&](const BwdOperands &cur, BwdOperands &nxt) {
                double lin = cur.blr - rho_lin * (cur.bv - cur.bg);  // q_i (state lanes) / r_i (input lanes), admm.cpp:77-80
                if constexpr (FAM) lin += cur.lx;
                const double w = is_x ? pcur : lin;
                pb -= 64;
                pl -= LRS;
                nxt.bg = pb[0]; nxt.bv = pb[VOFF];
                if constexpr (IREF) {
                    nxt.blr = q1; q1 = q2; q2 = q3; q3 = pl[-3 * LRS];
                } else {
                    nxt.blr = pl[0];
                }
                if constexpr (FAM) {
                    px_ -= 64;
                    nxt.lx = px_[0];
                }
                const double out = group_matvec<W, KT>(mb, w, cb);
                *pdst = out;  // d_i (input lanes)
                pdst -= ddec;
                pcur = lin + out;  // p_i (state lanes)
            };
            int i = N - 2;
            for (; i >= 1; i -= 2) {
                bstep(A, B);
                bstep(B, A);
            }
            if (i == 0) bstep(A, B);
        }
    }

    // ---- write-back: state for the next (warm-started) solve, solution, stats
    // the four norms of the last check (for get_stats), reduced once
    const double res_px = group_max<W>(is_x ? snap_pri : 0.0), res_pu = group_max<W>(is_u ? snap_pri : 0.0);
    const double res_dx = group_max<W>(is_x ? snap_dua : 0.0) * snap_rho, res_du = group_max<W>(is_u ? snap_dua : 0.0) * snap_rho;

    if (p.max_iter > 0 && inst_ok) {
        for (int kn = 0; kn < N; ++kn) {
            const int e = (kn + 1) * 64 + lane;
            gG[kn * 64 + lane] = sG[e];
            if (status != 1) gV[kn * 64 + lane] = sV[e];  // converged: HBM already holds the reference's stale v/z
            const double sol = sV[e];                       // solution = vnew / znew (admm.cpp:187-188, 204-205)
            if (is_x) p.sol_x[((size_t)inst * N + kn) * nx + r] = sol;
            if (is_u && kn < N - 1) p.sol_u[((size_t)inst * (N - 1) + kn) * nu + (r - nx)] = sol;
            if (is_u && kn == 0 && p.u0_host) p.u0_host[(size_t)inst * nu + (r - nx)] = sol;  // first controls straight to the host
            if (p.host_sol) {  // single-instance handle: the solution also goes straight into pinned host memory
                if (is_x) p.host_sol[(size_t)kn * nx + r] = sol;
                if (is_u && kn < N - 1) p.host_sol[(size_t)N * nx + (size_t)kn * nu + (r - nx)] = sol;
            }
        }
        if (is_u)
            for (int i = 0; i < N - 1; ++i) gD[i * dstride + dIdx] = sD[i * dstride + dIdx];
    }
    if (inst_ok && r == 0) {
        p.istats[inst * 2 + 0] = it_done;
        p.istats[inst * 2 + 1] = status;
        if (p.host_sol) {
            double *hs = p.host_sol + (size_t)N * nx + (size_t)(N - 1) * nu;
            hs[4] = (double)it_done;
            hs[5] = (double)status;
            if (res_valid) { hs[0] = res_px; hs[1] = res_dx; hs[2] = res_pu; hs[3] = res_du; }
        }
        if constexpr (ADAPT) p.rho_inst[inst] = rho;
        if (res_valid) {
            p.dstats[inst * 4 + 0] = res_px;
            p.dstats[inst * 4 + 1] = res_dx;
            p.dstats[inst * 4 + 2] = res_pu;
            p.dstats[inst * 4 + 3] = res_du;
        }
    }
