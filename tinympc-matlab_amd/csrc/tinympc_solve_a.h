// tinympc_solve_a.h -- layout A's kernels and their one launcher. The kernels share ONE body, tinympc_solve_a_body.h,
// which each of them includes with E naming its variant (the variants' additions sit behind `if constexpr`); each is compiled
// in its own source, as before: k_admm_solve (tinympc_solve.hip, the box path), k_admm_solve_fam (tinympc_solve_fam.hip, the
// cone / linear slack families), k_admm_solve_adapt (tinympc_solve_adapt.hip, adaptive rho), k_admm_solve_iref
// (tinympc_solve.hip, per-instance references), k_admm_solve_ibnd (tinympc_solve.hip, per-instance bounds) and k_admm_solve_imod
// (tinympc_imod_a.hip, per-instance models) and k_admm_solve_ifam (tinympc_ifam_a.hip, per-instance linear rows) and k_admm_solve_ifamk
// (tinympc_ifamk_a.hip, per-instance linear rows per knot). Each source instantiates
// launch_solve_a_e for its variant; launch_solve_a (tinympc_solve.hip) dispatches to them.
// (The body is not a __device__ __forceinline__ function: the compiler optimises such a function on its own before inlining
// it, and the box kernel's generated code then changes even for a verbatim move.)
#pragma once
#include "tinympc_device.h"
#include "tinympc_sweep.h"

namespace tinympc {

struct FwdOperands { double g, vold, lo, hi, dv, gc, gl; };  // (gc, gl: families only)
struct BwdOperands { double bg, bv, blr, lx; };              // (lx: families only)
// (per-knot linear rows: the rows of one knot slot a lane keeps in registers -- a | b | 1 / ||a||^2 of the first R rows; R = 1 and unused elsewhere)
// KNOT_REG_ROWS rows of the step's slot and as many of the next step's: 12 doubles per lane. Four and four -- the 24 doubles
// k_admm_solve_ifam keeps -- spill at 16 lanes: 8 to 42 vector registers in the <16, 16> forms, 5 scalars in the narrower ones (the
// fetch one step ahead keeps both sets AND the step's other operands alive at once); two and two leave every form without a spill.
constexpr int KNOT_REG_ROWS = 2;
template <int R> struct KnotRows { double a[R], b[R], in[R]; };
__device__ __forceinline__ double amax2(double m, double v) { return fmax(m, fabs(v)); }

// GMEM: the working copy of the state lives in p.scratch (HBM) instead of LDS -- the fallback for horizons
// that do not fit 160 KB of LDS. Same code, same results; the row-local operands then come from L2.
template <int W, int KT, bool TLDS, bool GMEM = false>
__global__ void __launch_bounds__(64) k_admm_solve(const SolveParams p);
template <int W, int KT, bool TLDS, bool GMEM = false>
__global__ void __launch_bounds__(64) k_admm_solve_fam(const SolveParams p);
template <int W, int KT, bool TLDS, bool GMEM = false>
__global__ void __launch_bounds__(64) k_admm_solve_adapt(const SolveParams p);
template <int W, int KT, bool TLDS, bool GMEM = false>
__global__ void __launch_bounds__(64) k_admm_solve_iref(const SolveParams p);
template <int W, int KT, bool TLDS, bool GMEM = false>
__global__ void __launch_bounds__(64) k_admm_solve_ibnd(const SolveParams p);
template <int W, int KT, bool TLDS, bool GMEM = false>
__global__ void __launch_bounds__(64) k_admm_solve_imod(const SolveParams p);
template <int W, int KT, bool TLDS, bool GMEM = false>
__global__ void __launch_bounds__(64) k_admm_solve_ifam(const SolveParams p);
template <int W, int KT, bool TLDS, bool GMEM = false>
__global__ void __launch_bounds__(64) k_admm_solve_ifamk(const SolveParams p);

template <SolveExt E, int W, int KT, bool TLDS, bool GMEM>
void (*kernel_a())(const SolveParams) {
    if constexpr (E == SolveExt::Box) return k_admm_solve<W, KT, TLDS, GMEM>;
    else if constexpr (E == SolveExt::Families) return k_admm_solve_fam<W, KT, TLDS, GMEM>;
    else if constexpr (E == SolveExt::Adaptive) return k_admm_solve_adapt<W, KT, TLDS, GMEM>;
    else if constexpr (E == SolveExt::InstRefs) return k_admm_solve_iref<W, KT, TLDS, GMEM>;
    else if constexpr (E == SolveExt::InstBounds) return k_admm_solve_ibnd<W, KT, TLDS, GMEM>;
    else if constexpr (E == SolveExt::InstModels) return k_admm_solve_imod<W, KT, TLDS, GMEM>;
    else if constexpr (E == SolveExt::InstFamilies) return k_admm_solve_ifam<W, KT, TLDS, GMEM>;
    else return k_admm_solve_ifamk<W, KT, TLDS, GMEM>;
}

template <SolveExt E, int W, int KT>
hipError_t launch_solve_a_t(const SolveParams &p, size_t lds_bytes, hipStream_t stream) {
    constexpr int IPW = 64 / W;
    const int groups = (p.batch + IPW - 1) / IPW;
    static size_t lds_set_t[16] = {0}, lds_set_f[16] = {0};
    if (p.scratch) {  // state in HBM scratch, tables from global memory, no dynamic LDS at all
        hipLaunchKernelGGL((kernel_a<E, W, KT, false, true>()), dim3(groups), dim3(64), 0, stream, p);
    } else {
        const auto kern = p.tables_in_lds ? kernel_a<E, W, KT, true, false>() : kernel_a<E, W, KT, false, false>();
        const hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void *>(kern), lds_bytes, p.tables_in_lds ? lds_set_t : lds_set_f);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, dim3(groups), dim3(64), lds_bytes, stream, p);
    }
    return hipGetLastError();
}

// The <W, KT> instantiations (choose_geometry); hipErrorInvalidValue for any other pair.
template <SolveExt E>
hipError_t launch_solve_a_e(const SolveParams &p, int W, int KT, size_t lds_bytes, hipStream_t stream) {
    if (W == 16 && KT == 8) return launch_solve_a_t<E, 16, 8>(p, lds_bytes, stream);
    if (W == 16 && KT == 12) return launch_solve_a_t<E, 16, 12>(p, lds_bytes, stream);
    if (W == 16 && KT == 16) return launch_solve_a_t<E, 16, 16>(p, lds_bytes, stream);
    if (W == 32 && KT == 32) return launch_solve_a_t<E, 32, 32>(p, lds_bytes, stream);
    if (W == 64 && KT == 64) return launch_solve_a_t<E, 64, 64>(p, lds_bytes, stream);
    return hipErrorInvalidValue;
}
extern template hipError_t launch_solve_a_e<SolveExt::Box>(const SolveParams &, int, int, size_t, hipStream_t);       // tinympc_solve.hip
extern template hipError_t launch_solve_a_e<SolveExt::Families>(const SolveParams &, int, int, size_t, hipStream_t);  // tinympc_solve_fam.hip
extern template hipError_t launch_solve_a_e<SolveExt::Adaptive>(const SolveParams &, int, int, size_t, hipStream_t);  // tinympc_solve_adapt.hip
extern template hipError_t launch_solve_a_e<SolveExt::InstRefs>(const SolveParams &, int, int, size_t, hipStream_t);  // tinympc_solve.hip
extern template hipError_t launch_solve_a_e<SolveExt::InstBounds>(const SolveParams &, int, int, size_t, hipStream_t);  // tinympc_solve.hip
extern template hipError_t launch_solve_a_e<SolveExt::InstModels>(const SolveParams &, int, int, size_t, hipStream_t);  // tinympc_imod_a.hip
extern template hipError_t launch_solve_a_e<SolveExt::InstFamilies>(const SolveParams &, int, int, size_t, hipStream_t);  // tinympc_ifam_a.hip
extern template hipError_t launch_solve_a_e<SolveExt::InstFamiliesKnots>(const SolveParams &, int, int, size_t, hipStream_t);  // tinympc_ifamk_a.hip

}  // namespace tinympc
