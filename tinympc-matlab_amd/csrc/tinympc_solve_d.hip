// tinympc_solve_d.hip -- k_admm_solve_d: the solve kernel in "layout D" (register-resident throughput layout), gfx950 FP64.
//
// Same algorithm and lane layout as the other solve kernels (tinympc_solve.hip has the reference citations:
// M1 solve admm.cpp:109-207 = F1 :25-35, S1 :43-59, D1 :65-69, L1 :75-83, R1 :89-107, C1 :196-197, B1 :13-20).
// What changes is where the ADMM state lives and, with it, how many wavefronts a SIMD runs:
//
//   layout B   G + D in LDS (33 KB per wave), V in HBM/L2        -> LDS caps a CU at 4 waves = ONE per SIMD; a lone wave
//              issues one VALU instruction per ~8 cycles on the dependent FP64 chain; 104 of 512 VGPRs in use.
//   layout D   the horizon is a COMPILE-TIME constant and both sweeps are fully unrolled, so every knot's dual g|y
//              has its own register pair (2*(N-1)+2 VGPRs) and the slack v|z is split between registers and LDS; LDS
//              holds only the feed-forward d (compact), part of v|z and one copy of the sweep operators per workgroup.
//              <= 256 VGPRs and <= 20 KB of LDS per wave -> 8 waves per CU = TWO per SIMD, whose FP64 chains
//              interleave. HBM is touched at entry and exit only (plus the conditional stale copy, below).
//              Horizons whose duals outgrow 256 registers run ONE wavefront per SIMD with all 512 (run-time specialised,
//              tinympc_jit.hip); a workgroup is four wavefronts where the LDS plan allows it, so that mid-size batches
//              spread over the CUs wavefront by wavefront (d_wpg below).
//
// Per sweep step the instruction stream is one asm block (tinympc_solve_d_chain.h): mov + (nx+nu) fused DPP FMAs +
// the 8-instruction row-local block going forward, (nx+nu) FMAs + 3 going backward (FMAs + 2 where references and bounds are
// constant over the horizon: FOLD in the body; forward step 0 has only its nu input columns: K0); no address arithmetic (LDS immediate
// offsets), no selects:
//   * the chain's columns k < nx read the state operand register, columns k >= nx the input-row operand register
//     (two different DPP sources), so [x_i; d_i] / [p_{i+1}; r_i] are never merged into one register;
//   * going backward every lane uses the SAME slot: slot s holds knot s+1 on state lanes and knot s on input lanes,
//     q_s is folded into the accumulator's start value (state lanes) instead of being added after the mat-vec;
//   * a converged instance keeps iterating as a zombie (no EXEC-masked region around the unrolled body); its state was
//     written back before the sweeps touch it again (see the control comment in the body).
// Run-time specialised variants (C++ between the asm blocks): FAM -- the cone / linear-inequality families --, and ADAPT --
// adaptive rho with rho per lane; see k_admm_solve_d_body.
// The sweep operators' rows (16 doubles per lane each) are re-read from LDS at the start of every sweep: holding both
// for the whole solve would cost 32 more VGPRs than the budget has.
//
// Reference semantics that need care are those of layout B (tinympc_solve_b.hip): per-instance termination,
// `iter % check_termination` with iter already incremented, the solution is vnew/znew, and a converged solve leaves
// the PREVIOUS iterate in v/z (admm.cpp:181-197) -- the stale copy goes to p.V2, written only in sweeps that can
// still end converged (decided on knot 0, after D_FIRST steps and then every D_GROUP steps; exact because the
// residual maxima only grow).
// A compiled-in specialisation (TINY_BUILTIN: __graft_entry__.HIP_BUILTINS_D) is the run-time specialisation's text -- one shape from
// -D options, one extern "C" entry point, no host side -- compiled by the build under the name TINY_BUILTIN_NAME; the build lints it,
// so it keeps the bare chain blocks (tinympc_solve_d_chain.h).
#if defined(TINY_BUILTIN) && !defined(TINY_JIT)
#define TINY_JIT 1
#endif
#ifndef TINY_JIT
#include <atomic>  // (host side only: the run-time compiler has no use for it)
#endif
#include <type_traits>

#include "tinympc_device.h"
#include "tinympc_sweep.h"

// Slot refill is a TEXTUAL variant of this file (TINY_REFILL: tinympc_solve_dr.hip includes it; -DTINY_JIT_REFILL=1 for the
// run-time specialisations), not a template parameter of the plain kernels: as one, the non-refill instantiation kept its
// semantics but not its code, and lost 2.6 % (profiles/r03_dgroup_ab.txt). What it had lost was found afterwards -- its sweep
// chains had moved off the 8-byte grid by one 4-byte instruction, see D_AL in tinympc_solve_d_chain.h, which now puts every
// chain on the grid by construction; the variant stays textual all the same: the plain translation unit preprocesses to
// exactly the text it had before the variant existed.
#ifndef TINY_REFILL
#if defined(TINY_JIT_REFILL) && TINY_JIT_REFILL
#define TINY_REFILL 1
#else
#define TINY_REFILL 0
#endif
#endif

// Lean sweeps are a textual variant in the same way (TINY_LEAN: tinympc_lean_d.hip includes this file): an iteration whose
// residuals nothing can read -- no termination check falls on it, or the tolerances cannot be met and a later check overwrites its
// snapshot -- runs a forward sweep without the residual maxima (Step::fwd_*_nores), without the "can this sweep still converge" tests
// and without R1. With reachable = both tolerances > 0 (a launch constant),
//     need_res(it1) = check(it1) && (reachable || it1 + check_termination > max_iter)
// and only the iterations with need_res run the sweep of the plain kernel. The lean iteration is an innermost loop of its own (one
// forward, one backward sweep: what the register allocator sees in the plain kernel, less the residuals' registers); the iteration
// with residuals follows it in the enclosing loop. Box path only; results are bit-identical to the plain kernel's.
#ifndef TINY_LEAN
#define TINY_LEAN 0
#endif
#if TINY_LEAN && (TINY_REFILL || defined(TINY_JIT))
#error "TINY_LEAN: compiled-in plain kernels only"
#endif
// ... and the lean kernels have a textual variant of their own (TINY_LEAN_START: tinympc_lstart_d.hip sets it with TINY_LEAN; new
// symbols k_admm_solve_d_lean_start, k_admm_solve_d_gbnd_lean_start, launch_solve_d_lean_start), two changes to the lean inner loop that
// keep every instruction of its arithmetic, its order and its operands:
//   LDS start  a forward step's accumulator does not start as a VALU copy of cf: cf sits in a 16-double table behind the shared
//              operators and a ds_read issued one block ahead, beside the read of d, fills the accumulator (Step::fwd_*_start). Step 0
//              keeps its copy of c0, which is per instance. (-DTINY_LEAN_NO_LDS_START: without it, for the A/B)
//   hoist      nothing inside the lean inner loop can change pending, active or final_round -- only an iteration with residuals sets
//              them --, so the write-back test and the "all instances done" exit are evaluated once in front of the inner loop, and
//              it_done is set once behind it: a lean round is fair_share_priority, forward sweep, backward sweep, back edge.
//              (-DTINY_LEAN_NO_HOIST: without it)
#ifndef TINY_LEAN_START
#define TINY_LEAN_START 0
#endif
#if TINY_LEAN_START && !TINY_LEAN
#error "TINY_LEAN_START: a variant of the lean kernels"
#endif
#if TINY_LEAN_START && !defined(TINY_LEAN_NO_LDS_START)
#define TINY_LDS_START 1
#else
#define TINY_LDS_START 0
#endif
#if TINY_LEAN_START && !defined(TINY_LEAN_NO_HOIST)
#define TINY_LEAN_HOIST 1
#else
#define TINY_LEAN_HOIST 0
#endif
// ... and the lean-start kernels have a textual variant in turn (TINY_LEAN_TRIM: tinympc_ltrim_d.hip sets it with the two above; new symbols
// k_admm_solve_d_lean_trim, k_admm_solve_d_gbnd_lean_trim, launch_solve_d_lean_trim). The lean loop's arithmetic is at its floor; what this
// variant takes out of a lean round are instructions BESIDE the arithmetic, which the results cannot see (docs/NOTEBOOK.md section 15 has
// what was tried; one part passed its A/B):
//   dstore  the backward sweep stored d_s for the input lanes of live instances by narrowing EXEC around each store (two scalar
//           instructions per step). `active` cannot change inside a run of lean rounds, so the mask is turned into a per-lane ADDRESS in
//           front of the run: input lanes of live instances keep the address of their d, every other lane gets a dump address, and the
//           49 stores of a round are plain ds_write_b64. A dump address is a live instance's column of d one or two rows UP: with the
//           step's immediate offset the lane writes row s-1 or s-2 of that column at step s, and the column's own lane overwrites it at
//           step s-1 / s-2, which comes later (the sweep runs from the last row down, LDS operations of a wavefront complete in order);
//           rows -1 and -2 are D_DUMP_DOUBLES spare doubles in front of d. No row of an instance that is not live is ever touched.
//           (-DTINY_TRIM_NO_DSTORE: without it)
#ifndef TINY_LEAN_TRIM
#define TINY_LEAN_TRIM 0
#endif
#if TINY_LEAN_TRIM && !(TINY_LEAN_START && TINY_LEAN_HOIST && TINY_LDS_START)
#error "TINY_LEAN_TRIM: a variant of the lean-start kernels (LDS starts and hoisted control)"
#endif
#if TINY_LEAN_TRIM && !defined(TINY_TRIM_NO_DSTORE)
#define TINY_TRIM_DSTORE 1
#define D_DUMP_DOUBLES(nu) (2 * 4 * (nu))  // two rows of d (4 instances x nu inputs) in front of a wavefront's d: see `dstore` above
#else
#define TINY_TRIM_DSTORE 0
#endif
// ... and the trimmed kernels have a textual variant once more (TINY_LEAN_SHARE: tinympc_lshare_d.hip sets it with the three above; new
// symbols k_admm_solve_d_lean_share, k_admm_solve_d_gbnd_lean_share, launch_solve_d_lean_share). In a lean round the two values a slot
// stores are never alive together: d_s lives from backward step s to forward step s of the NEXT round, the slack v_s from forward step s
// (which writes it; a lean step does not read the old one) to the tail of backward step s+2 (t = v - g). A backward step leaves d_s on
// the input lanes of its accumulator [p_s | d_s], the lanes the forward chain's input columns read. So for the NVR slots whose slack is a
// register, that register holds a_s and v_s in turn:
//   backward  the block of a register slot accumulates in Vr[s-VL] itself -- the previous block's tail writes the start value there, two
//             blocks after the tail that consumed v_s --, the next block reads its state operand from it, and d_s is not stored;
//   forward   the step of a register slot takes Vr[q-VL] as its d operand and writes the clamp into it behind the chain's last read
//             (fwd_reg_start's text, one register for both operands); no d read is issued for it.
//   waits     the backward blocks of the register slots down to VL+3 (constant tables) have no LDS instruction around them and would need
//             no s_waitcnt. A form without it was built and is NOT in: between two asm statements with nothing in between the compiler
//             puts an `s_nop 0` of its own (one wait state between an asm statement's results and the next one's operands), so the block
//             trades its wait for a nop, and the A/B could not tell the two builds apart (docs/NOTEBOOK.md section 18).
// A run of n lean rounds is: load d_s of the register slots from LDS into Vr[] (the old slack is dead: the first forward sweep overwrites
// it unread, and the control block in front of the run has done every pending write-back); n-1 shared rounds; one round with the
// shared forward and the trimmed kernels' backward sweep (scratch accumulator, every d_s stored through the dstore addresses, Vr[]
// untouched), after which Vr[] is the slack and LDS holds all of d, as the iteration with residuals and the final write-back expect.
// Instances that are not live: inside a run their lanes' Vr[] change (they hold what a zombie's backward sweep computed), where the
// trimmed kernels kept re-reading the frozen d from LDS. Nothing reads those registers: a zombie's state was written back by the control
// block in front of the run (pending is false inside it, `active` is fixed for it), the stale copy and the dual residual are taken only
// in iterations with residuals and only for live instances, and the final write-back stores live or pending instances only. Their d in
// LDS is never written: the last round's stores go through aDw like every lean round's. The arithmetic of a live instance keeps every
// instruction, its operands' values and its order (one exception on a dead value: with VL = 0 the tail of backward block 1 forms its
// "any finite t" from rhom instead of v_0, whose register is the block's output).
#ifndef TINY_LEAN_SHARE
#define TINY_LEAN_SHARE 0
#endif
#if TINY_LEAN_SHARE && !(TINY_LEAN_TRIM && TINY_TRIM_DSTORE)
#error "TINY_LEAN_SHARE: a variant of the trimmed lean kernels (with their dstore addresses)"
#endif
// ... and the shared kernels have a textual variant (TINY_LEAN_PARK: tinympc_lpark_d.hip sets it with the four above; new symbols
// k_admm_solve_d_lean_park, k_admm_solve_d_gbnd_lean_park, launch_solve_d_lean_park; quadrotor N=50 with constant tables only -- the
// other shapes have no LDS slot). The kernel stands at 254 VGPRs, which is why VL is 25, but the shared round -- the loop a run spends
// its time in -- names only 217 of them: the rest hold temporaries of the other round bodies and values the loop does not use. So
// INSIDE a run a second split holds: VLR = VL - TINY_PARK_SLOTS LDS slots, and the slots VLR..VL-1 are register slots of a second
// array, Vx[], that lives from the run's entry to the last round's forward sweep. Each converted slot saves the four LDS instructions
// a round spends on it (slack store and d read going forward, slack read and d store going backward).
//   entry     behind the control block and the dstore addresses: d_s of ALL NS - VLR register slots comes from LDS into Vr[] and Vx[].
//   shared    (form 3) a slot >= VLR takes the register-slot text of TINY_LEAN_SHARE, on Vx[s-VLR] below VL; the boundary block is VLR.
//   last      (form 4) the forward step of a converted slot takes Vx[q-VLR] as its d operand and hands its clamp to the slot's LDS slack
//             row (fwd_lds_start's text and the store that always followed it); behind the forward sweep Vx[] is dead. The backward
//             sweep is the trimmed kernels', on VL: Vr[] is the slack, LDS holds all of d and the slack of the slots below VL.
// Why this is the same computation. (1) The old slack of a converted slot is dead at entry for the reason Vr[]'s is: the first forward
// sweep of a run writes v_s without reading it -- into Vx[] (form 3) or into the LDS row (form 4) --, and the control block in front of
// the run has written every pending instance back (vget reads the LDS row there, before the entry). Between the entry and the last
// round's forward sweep the LDS slack rows of the converted slots are stale and nothing reads them: a shared backward block takes v_s of
// a slot >= VLR from its register, and nothing but sweeps runs inside a run. (2) The d rows VLR..NS-1 in LDS are not read inside a run
// either (forward steps of register slots issue no d read); the last round's backward sweep rewrites all of them for live instances.
// (3) Instances that are not live: as with Vr[], their lanes' Vx[] hold what a zombie's sweeps computed, and nothing reads it -- Vx[] is
// dead behind the run; their LDS slack rows of converted slots are written by the last round's forward sweep exactly as every lean round
// of the parent wrote them (the store is unconditional there too); their d rows below VLR are never written (aDw). (4) Dump lanes: a
// dump lane writes row s-1 or s-2 of a live column at a block s that stores. In a shared round those are the blocks below VLR, so the
// dump rows are -2..VLR-2, each overwritten by its own column's lane later in the same sweep (or spare): `dstore`'s argument with VLR
// for VL. In the last round every block stores, as in the parent. (5) Parked values. The loop needs 217 + 24 = 241 registers; of the
// values that live across a run without being used in it, three doubles per lane -- the residual snapshot snap_pri, snap_dua and the
// pair (status, it_done) -- go to LDS at the entry and come back in the last round, between its forward sweep (behind which Vx[] is
// dead) and its backward sweep; three more are rebuilt where they are used (the 64-bit constants of the "can still converge" test:
// the test on 32-bit halves; the address of knot 0's stale copy and the instance's 64-bit index: from an opaque copy of the lane).
// The parked rows are the d rows VLR..VLR+11 of the wavefront taken as [3][64 lanes]: the entry has just read them into registers,
// no shared round reads or writes them (2), and the last round's backward sweep, which rewrites them for every live instance, runs
// behind the reload. Instances that are not live keep parked bits in those rows of their d. Nothing reads them: their write-back
// happened in front of the entry (pending is false inside a run), their lanes' arithmetic is never read (as in TINY_LEAN_SHARE; a DPP
// chain stays inside its 16-lane row), and an instance that stops being live LATER was live in this run and had its rows rewritten.
#ifndef TINY_LEAN_PARK
#define TINY_LEAN_PARK 0
#endif
#if TINY_LEAN_PARK && !TINY_LEAN_SHARE
#error "TINY_LEAN_PARK: a variant of the shared lean kernels"
#endif
#if TINY_LEAN_PARK && !defined(TINY_PARK_SLOTS)
#define TINY_PARK_SLOTS 12  // LDS slots that become register slots inside a run (VL - VLR)
#endif

#define TINY_STR2(x) #x
#define TINY_STR(x) TINY_STR2(x)
namespace tinympc {
template <int NX, int NU>
struct DStep;  // specialised per (nx, nu) by tinympc_solve_d_chain.h
}  // namespace tinympc

// The (nx, nu) pairs compiled into the library: quadrotor, cartpole, rocket landing (BASELINE.json configs 2-5).
#ifdef TINY_JIT  // run-time specialisation (tinympc_jit.hip): exactly one (nx, nu, N), from -D options
#define D_NX TINY_JIT_NX
#define D_NU TINY_JIT_NU
#include "tinympc_solve_d_chain.h"
#else
#define D_NX 12
#define D_NU 4
#include "tinympc_solve_d_chain.h"
#define D_NX 4
#define D_NU 1
#include "tinympc_solve_d_chain.h"
#endif

namespace tinympc {

template <int I, int E, class F>
__device__ __forceinline__ void static_for(F &&f) {
    if constexpr (I < E) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, E>(f);
    }
}

// ---- LDS plan per workgroup, in doubles: operators [2][16 k][16 r] | tables (!CT) | per wave: V[VL][64], D[(N-1)*4*nu]
// (IMOD: no shared operators; per wave V | D | its four instances' operator blocks)
constexpr int D_OPS_DOUBLES = 2 * 16 * 16;
// (TINY_LDS_START: cf per lane row, behind the shared operators -- the accumulator starts of the lean forward steps; this variant only)
constexpr int D_START_DOUBLES = TINY_LDS_START ? 16 : 0;
#ifdef TINY_D_GROUP
constexpr int D_GROUP = TINY_D_GROUP;  // (experiments)
constexpr int D_FIRST = TINY_D_FIRST;
#else
// Forward steps between two "can this sweep still converge" tests: one test on knot 0 alone, the next after D_FIRST
// steps (a sweep that cannot converge has then copied D_FIRST slots of stale iterate at most), then every D_GROUP steps.
// Each test is a scheduling boundary of the unrolled sweep; 4 | 23 measured best of the splits tried on the headline
// (profiles/r03_dgroup_ab.txt), forced iterations and converging batch alike.
#if TINY_REFILL
// (the slot-refill variant runs converging batches: finer groups cut a sweep's stale copies sooner -- 4 | 12 measured best of
// eight splits on the 65,536-instance converging batch, 10.7 against 10.85 ms with 4 | 23; profiles/r03_refill_probe.txt)
constexpr int D_GROUP = 12;
constexpr int D_FIRST = 4;
#else
constexpr int D_GROUP = 23;
constexpr int D_FIRST = 4;
#endif
#endif
#ifdef TINY_JIT_VREG
constexpr int D_VREG_MAX = TINY_JIT_VREG;  // chosen by the host from its register estimate
#else
constexpr int D_VREG_MAX = 24;
#endif    // slack knots kept in registers (the rest goes to LDS)
constexpr int D_LDS_PER_CU = 160 * 1024;
__host__ __device__ constexpr int d_d_doubles(int nu, int N) { return ((N - 1) * 4 * nu + 1) & ~1; }
__host__ __device__ constexpr int d_tab_doubles(int N) { return 3 * (N + 2) * 16 + 16; }
constexpr int D_FAM_DOUBLES = 3 * MAX_LIN_ROWS * 16;  // FAM: a_k | b_k | 1/||a_k||^2 of the linear rows, per lane row
constexpr int D_ADAPT_DOUBLES = 5 * 16 * 16;         // ADAPT: dMf | dMb | [A'; B'] | Pinf | dPinf, transposed like the operators
// IMOD: the operators are per WAVEFRONT, one [2][16 k][16 r] block for each of its four instances, and no workgroup-shared copy. A row
// read is a 64-bit read per lane, served in two groups of 32 lanes = two instances, bank = (byte address / 4) mod 64: the two blocks
// of a group must lie an odd multiple of 32 banks = 16 doubles apart -- 512 + 16.
constexpr int D_IMOD_STRIDE = D_OPS_DOUBLES + 16;
constexpr int D_IMOD_WAVE_DOUBLES = 4 * D_IMOD_STRIDE;
// number of slack slots in LDS; -1 if the shape does not fit the plan (cu_waves wavefronts per CU: 8, or 4 for the
// long-horizon plan with one wavefront per SIMD and 512 registers)
// (ilin: the row count of the per-instance linear-row form, 0 otherwise -- 3 ilin vectors of 64 doubles per WAVEFRONT in place of the
// workgroup's D_FAM_DOUBLES; knots: the slots of its per-knot form, N of them, each 3 ilin vectors -- 0: rows constant over the horizon)
__host__ __device__ constexpr int d_ilin_wave_doubles(int ilin, int knots) { return 3 * ilin * 64 * (knots > 0 ? knots : 1); }
// (itraj: the per-instance trajectory form -- the wavefront's own linref rows, table_rows(N) = N + 2 vectors of 64 doubles, SolveParams::iref_lr's block)
__host__ __device__ constexpr int d_itraj_wave_doubles(bool itraj, int N) { return itraj ? (N + 2) * 64 : 0; }
// (ikbnd: the per-knot bounds form -- the wavefront's own clamp rows, lo and hi, 2 (N + 2) vectors of 64 doubles, SolveParams::ibnd's two blocks)
__host__ __device__ constexpr int d_ikbnd_wave_doubles(bool ikbnd, int N) { return ikbnd ? 2 * (N + 2) * 64 : 0; }
__host__ __device__ constexpr int d_vl(int nu, int N, bool ct, int wpg, int cu_waves = 8, bool fam = false, bool adapt = false, bool imod = false, int ilin = 0,
                                       int knots = 0, bool itraj = false, bool ikbnd = false) {
    const int ns = N - 1;
    const int wg_doubles = D_LDS_PER_CU / 8 * wpg / cu_waves - (imod ? 0 : D_OPS_DOUBLES + D_START_DOUBLES) - (ct ? 0 : d_tab_doubles(N)) - (fam && !ilin ? D_FAM_DOUBLES : 0) - (adapt ? D_ADAPT_DOUBLES : 0);
#if TINY_TRIM_DSTORE
    const int wave_doubles = wg_doubles / wpg - d_d_doubles(nu, N) - D_DUMP_DOUBLES(nu) - (imod ? D_IMOD_WAVE_DOUBLES : 0);
#else
    const int wave_doubles = wg_doubles / wpg - d_d_doubles(nu, N) - (imod ? D_IMOD_WAVE_DOUBLES : 0) - d_ilin_wave_doubles(ilin, knots) - d_itraj_wave_doubles(itraj, N) -
                             d_ikbnd_wave_doubles(ikbnd, N);
#endif
    if (wave_doubles < 0) return -1;
    const int vlmax = wave_doubles / 64;
    const int want = ns > D_VREG_MAX ? ns - D_VREG_MAX : 0;
    return want <= vlmax ? want : -1;
}
__host__ __device__ constexpr size_t d_lds_bytes(int nu, int N, bool ct, int wpg, int vl, bool fam = false, bool adapt = false, bool imod = false, int ilin = 0,
                                                 int knots = 0, bool itraj = false, bool ikbnd = false) {
    return sizeof(double) * ((size_t)(imod ? 0 : D_OPS_DOUBLES + D_START_DOUBLES) + (ct ? 0 : d_tab_doubles(N)) + (fam && !ilin ? D_FAM_DOUBLES : 0) + (adapt ? D_ADAPT_DOUBLES : 0) +
#if TINY_TRIM_DSTORE
                             (size_t)wpg * (vl * 64 + D_DUMP_DOUBLES(nu) + d_d_doubles(nu, N) + (imod ? D_IMOD_WAVE_DOUBLES : 0)));
#else
                             (size_t)wpg * (vl * 64 + d_d_doubles(nu, N) + (imod ? D_IMOD_WAVE_DOUBLES : 0) + d_ilin_wave_doubles(ilin, knots) + d_itraj_wave_doubles(itraj, N) +
                                            d_ikbnd_wave_doubles(ikbnd, N)));
#endif
}

// LDS traffic of the sweeps: WHERE a read is issued is this file's decision, not the scheduler's (see tinympc_solve_d_chain.h) -- reads
// are issued one block ahead and retired by the wait behind the block; both in a form the compiler tracks (tinympc_sweep.h:
// lds_read_issued_here / lds_reads_landed). Writes carry no result and stay plain asm.
__device__ __forceinline__ unsigned lds_addr(const double *p) { return lds_address(p); }
template <int OFF>
__device__ __forceinline__ double lds_read_async(unsigned addr) {  // the value is valid after the next lds_reads_landed()
    return lds_read_issued_here<OFF>(addr);
}
template <int OFF>
__device__ __forceinline__ void lds_write_async(unsigned addr, double v) {
    static_assert(OFF >= 0 && OFF < 65536, "ds offset field is 16 bits");
    asm volatile("ds_write_b64 %0, %1 offset:%2" ::"v"(addr), "v"(v), "n"(OFF) : "memory");
}
// Store for the lanes of `mask` only, without a branch: EXEC is narrowed around the one instruction by two scalar
// instructions (a branch around the store would put a label between two sweep blocks -- one more taken-or-not decision per
// step, and a branch target the ISA lint could not see through).
template <int OFF>
__device__ __forceinline__ void lds_write_masked(unsigned addr, double v, unsigned long long mask) {
    static_assert(OFF >= 0 && OFF < 65536, "ds offset field is 16 bits");
    unsigned long long saved;
    asm volatile("s_and_saveexec_b64 %[sv], %[m]\n\t"
                 "ds_write_b64 %[a], %[v] offset:%[o]\n\t"
                 "s_mov_b64 exec, %[sv]"
                 : [sv] "=&s"(saved)
                 : [m] "s"(mask), [a] "v"(addr), [v] "v"(v), [o] "n"(OFF)
                 : "memory", "scc");
}
__device__ __forceinline__ void lds_wait() {
    lds_reads_landed();
    asm volatile("" ::: "memory");
}
// ... and the point where the compiler retires ITS OWN reads of the sweep's operator rows: left alone it waits for them in
// front of the first block that uses them, i.e. right behind the asynchronous reads issued for the second block -- a full
// LDS latency in every sweep. (The empty asm makes the rows operands of THIS point.)
__device__ __forceinline__ void lds_wait_ops(double (&m)[16]) {
    lds_reads_landed();
#ifdef TINY_D_NO_OPS_WAIT
    asm volatile("" ::: "memory");
#else
    asm volatile(""
                 : "+v"(m[0]), "+v"(m[1]), "+v"(m[2]), "+v"(m[3]), "+v"(m[4]), "+v"(m[5]), "+v"(m[6]), "+v"(m[7]), "+v"(m[8]), "+v"(m[9]),
                   "+v"(m[10]), "+v"(m[11]), "+v"(m[12]), "+v"(m[13]), "+v"(m[14]), "+v"(m[15])
                 :
                 : "memory");
#endif
}

// `bad` = ballot of lanes whose row already rules out convergence in this sweep, `live` = ballot of the lanes that
// are still iterating. True if some live instance (16-lane row) has no bad lane.
// (no short-circuit evaluation: four scalar compares instead of a chain of branches in every sweep)
__device__ __forceinline__ bool wave_may_converge_d(unsigned long long bad, unsigned long long live) {
    int any = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned b = (unsigned)(bad >> (j * 16)) & 0xffffu, l = (unsigned)(live >> (j * 16)) & 0xffffu;
        any |= (int)(l != 0u) & (int)(b == 0u);
    }
    return any != 0;
}
// The same test on the 32-bit halves of the two ballots (the per-instance linear-row form: the 64-bit form above compares two of its
// rows against 64-bit constants in the VALU, which the allocator keeps in vector registers across the iteration loop -- with the
// families' register pairs per knot they ended up in its spill slots; here every compare is a 32-bit scalar one).
__device__ __forceinline__ bool wave_may_converge_d32(unsigned long long bad, unsigned long long live) {
    unsigned b0 = (unsigned)bad, b1 = (unsigned)(bad >> 32), l0 = (unsigned)live, l1 = (unsigned)(live >> 32);
    asm("" : "+s"(b0), "+s"(b1), "+s"(l0), "+s"(l1));  // (opaque halves: the optimiser otherwise folds the tests back into 64-bit compares)
    const int any = ((int)((l0 & 0xffffu) != 0u) & (int)((b0 & 0xffffu) == 0u)) | ((int)((l0 >> 16) != 0u) & (int)((b0 >> 16) == 0u)) |
                    ((int)((l1 & 0xffffu) != 0u) & (int)((b1 & 0xffffu) == 0u)) | ((int)((l1 >> 16) != 0u) & (int)((b1 >> 16) == 0u));
    return any != 0;
}
// Branches that are almost never taken (write-back, stale copies): the compiler moves their bodies out of the sweep's
// straight line. A TAKEN branch costs a wavefront ~110 cycles of instruction fetch (tools/microbench_fp64_step.hip, loops
// against straight-line code), so the common path should be the fall-through.
#ifdef TINY_D_NO_RARE
#define TINY_RARE(c) (c)
#else
#define TINY_RARE(c) __builtin_expect(!!(c), 0)
#endif

// FAM: the second-order-cone and linear-inequality slack families of k_admm_solve_fam (PARITY UNPINNED, see there) ride on
// the forward step exactly as in the latency kernel (tinympc_solve_c.hip): every knot carries two more duals gc|yc, gl|yl
// (persistent: the HBM arrays GC / GL) and the families' linear-cost term lx (forward -> backward), all in registers.
// Run-time specialised only (tinympc_jit.hip, -DTINY_JIT_FAM=1): 10 VGPRs per knot instead of 4, so short horizons.
// ADAPT: adaptive rho (admm.cpp:117-174, rho_benchmark.cpp) exactly as in k_admm_solve_adapt -- rho is PER INSTANCE (a lane
// variable, persistent in p.rho_inst), the lane's operator rows are (base row) + (rho - rho0) * (derivative row) rebuilt from
// LDS at every sweep, and every fifth iteration the four norms of the reference's dense KKT system ride on the forward sweep
// (one extra mat-vec per step). Run-time specialised only (-DTINY_JIT_ADAPT=1), not together with the families.
// HOSTX: the batched zero-copy tick (x0 read from pinned host memory and mirrored, first controls written to pinned host memory). A variant
// of its own: as run-time branches in the rare paths of the one kernel the two stores cost the sweeps 3.6 % (1.72 -> 1.78 ms: the
// pointers' scalar registers, live across the unrolled iteration loop).
#if TINY_REFILL
// REFILL: slot refill (SolveParams::refill_next). The launch is one resident set of wavefronts; every 16-lane row counts its OWN
// iterations, and a row whose instance has finished (converged, or max_iter) is written back -- state, solution, statistics -- and
// loaded with the next instance of the batch, cold or warm, while the other three rows of the wavefront keep iterating. The
// arithmetic of an instance is that of the plain kernel (bit-identical results: tests/test_hip_parity.py); what changes is that
// a wavefront's time is the sum of what its rows worked, not four times its slowest instance.
// REFILL with IGOAL (the per-instance goal form of the box path, k_admm_solve_d_refill_gbnd): lr_c, pNref, lo_c and hi_c belong to the
// row's CURRENT instance -- loaded per lane at kernel start, reloaded with the folded accumulator start where a row takes an instance.
// REFILL with ITRAJ and / or IKBND (forms of the goal form, box path; run-time specialised, k_builtin_d_quadrotor50_traj_refill compiled
// in): the wavefront stages its FIRST group's linref / clamp rows at kernel start as the plain form does; a row that takes an instance
// reloads the lane constants its form has (pNref, lo_c, hi_c with ITRAJ; pNref and, without ITRAJ, lr_c with IKBND) and restages its own
// 16-lane column of those rows from the new instance's column of ITS group's block. FOLD is off in both forms: nothing is recomputed.
template <int NX, int NU, int N, bool CT, int WPG, int VL, bool FAM = false, bool ADAPT = false, bool TWO_PER_SIMD = true, bool HOSTX = false,
          bool REFILL = false, bool IGOAL = false, bool IMOD = false, int ILIN = 0, bool ICONE = false, bool IKNOT = false, bool ITRAJ = false, bool IKBND = false>
#else
// IGOAL: the per-instance goal form (every instance's references and bounds constant over the horizon; k_admm_solve_d_gbnd) -- the
// four table constants lr_c, pNref, lo_c and hi_c come per lane from SolveParams::iref_lr / iref_pn / ibnd ([instance][16], ibnd's hi
// at groups*64) instead of the shared table. The same registers, loaded from elsewhere; nothing else changes.
// IMOD: the per-instance model form (tinympc_set_model_batch; the goal form with SolveParams::ops [batch][ops_doubles(W, KT)]) -- the
// two sweep operators a lane reads its rows from are its INSTANCE's, staged by its wavefront into the wavefront's own LDS region, and
// cf, cb, c0 and the folded start value come from the instance's block. The per-lane arithmetic is the goal kernel's.
// ILIN: the per-instance linear-row form of the families (tinympc_set_linear_constraints_batch after tinympc_prepare; ILIN = the mode's
// row count nl, 0: off) -- the families' code reads a_k | b_k | 1/||a_k||^2 of the lane's own INSTANCE from SolveParams::ilin,
// [group][slopes | 3 nl rows][64], which every wavefront stages into an LDS region of its own; the shared sLin block does not exist. The
// ICONE (with ILIN): the cone slope mu is the lane's instance's too (tinympc_set_cone_slopes_batch: the store's round-0 vector; a handle
// without linear rows runs the form with one absent row); without it the form's code is what it was before the slopes' half existed. Cones, role and the enable flags stay those of the shared description, the four table constants come per lane as in the goal form
// (layout A's variant of the mode always runs on per-instance reference and clamp rows). The per-element arithmetic is FAM's.
// IKNOT (with ILIN): the rows of every KNOT (tinympc_set_linear_constraints_knots_batch after tinympc_prepare) -- the group's block of
// SolveParams::ilin holds N slots of 3 nl vectors in the forward sweep's own skew (k_build_inst_lin_knots: slot 0 is knot 0 on the state
// lanes, slot q+1 what forward step q finishes), the third vector already 1 / ||a_k||^2. The wavefront stages the whole block, verbatim,
// and `families` reads the slot of its call: the horizon is unrolled, so a slot is a compile-time offset of the same three reads.
// ITRAJ (with IGOAL): per-instance reference TRAJECTORIES and tracks (tinympc_set_x_ref_batch / _u_ref_batch / the track verbs after
// tinympc_prepare) -- SolveParams::iref_lr is layout A's store, [group][N + 2][64] in this kernel's lane order (k_build_inst_tables: row
// k + 1 = knot k), and the wavefront stages its group's block, verbatim, into an LDS region of its own. The backward sweep reads the
// linref of slot S there, the row the shared !CT form reads in the workgroup's table, one block ahead like the slack; bounds and pNref
// stay the goal form's (constant over the horizon, per lane). FOLD needs references constant over the horizon: off.
// ITRAJ with ILIN (ICONE and IKNOT as they are): the per-instance families on per-instance trajectories -- both blocks are staged, the
// trajectory rows behind the linear rows, and every linref of the backward sweep is the row's read plus the families' LX of its slot.
// IKBND (with IGOAL, box path; with or without ITRAJ): box bounds per knot AND per instance (tinympc_set_bound_constraints_batch with one
// column per knot after tinympc_prepare, or shared per-knot bounds beside per-instance trajectories) -- SolveParams::ibnd is layout A's
// store, lo [group][N + 2][64] | hi [group][N + 2][64] in this kernel's lane order (k_build_inst_tables: row k + 1 = knot k), and the
// wavefront stages its group's two blocks, verbatim, into an LDS region of its own (behind its linref rows where the form has both). The
// forward sweep reads the clamp of slot q there, the rows the shared !CT form reads in the workgroup's table, one step ahead like d; knot
// 0's clamp is row 1. References, pNref and (without ITRAJ) lr_c stay the goal form's. FOLD is off, as in the shared !CT form: the
// arithmetic of an instance is that form's, bit for bit.
template <int NX, int NU, int N, bool CT, int WPG, int VL, bool FAM = false, bool ADAPT = false, bool TWO_PER_SIMD = true, bool HOSTX = false,
          bool REFILL = false, bool IGOAL = false, bool IMOD = false, int ILIN = 0, bool ICONE = false, bool IKNOT = false, bool ITRAJ = false, bool IKBND = false>
#endif
__device__ __forceinline__ void k_admm_solve_d_body(const SolveParams &p, double *smem) {
    static_assert(!(FAM && ADAPT), "adaptive rho and the constraint families exclude each other (as in the C ABI)");
    static_assert(!IMOD || (IGOAL && CT && !FAM && !ADAPT && !REFILL && !HOSTX && !TINY_LEAN),
                  "per-instance models: the goal form of the box path (its rows are always built per instance), plain sweeps");
    static_assert(!ICONE || ILIN > 0, "per-instance cone slopes: with the per-instance rows' form (one absent row where there are none)");
    static_assert(!IKNOT || ILIN > 0, "rows per knot: a form of the per-instance rows");
    static_assert(!ITRAJ || (IGOAL && CT && FAM == (ILIN > 0) && !ADAPT && !IMOD && (!REFILL || ILIN == 0) && !HOSTX && !TINY_LEAN),
                  "per-instance trajectories: the goal form of the box path (plain sweeps or slot refill), or of the per-instance families (bounds constant over the horizon; plain sweeps)");
    static_assert(!IKBND || (IGOAL && CT && !FAM && ILIN == 0 && !ADAPT && !IMOD && !HOSTX && !TINY_LEAN),
                  "per-knot bounds per instance: the goal form of the box path (references constant over the horizon or per-instance trajectories), plain sweeps or slot refill");
    static_assert(ILIN == 0 || (ILIN > 0 && ILIN <= MAX_LIN_ROWS && FAM && IGOAL && CT && !ADAPT && !IMOD && !REFILL && !HOSTX && !TINY_LEAN),
                  "per-instance linear rows: the families' variant in the goal form (references and bounds constant over the horizon), plain sweeps");
#if TINY_REFILL
    static_assert(!REFILL || (!FAM && !ADAPT && !HOSTX), "slot refill: box-constrained path only");
#endif
    // this wavefront's slot on its SIMD (HW_REG_HW_ID bits 3:0): the two wavefronts of a SIMD sit in different slots
    const int simd_slot = TWO_PER_SIMD ? simd_slot_id() : 0;
    constexpr int W = 16, IPW = 4, NXU = NX + NU, NS = N - 1, DS = IPW * NU, NVR = NS - VL;
    constexpr int KT = NXU <= 8 ? 8 : NXU <= 12 ? 12 : 16;  // row stride of p.ops (choose_geometry)
    constexpr int TOFF = (N + 2) * W;
    static_assert(NS >= 3 && VL >= 0 && VL <= NS, "layout D: N >= 4");
    using Step = DStep<NX, NU>;
    // Work that does not change within a launch, taken out of the sweeps (box path only: the families' and adaptive rho's code is
    // untouched). K0: x_0 is fixed, so the state columns of forward step 0 are summed once into its accumulator start c0 (not in the
    // slot-refill variant: it sits at 256 registers with its rare paths in scratch, and the two registers of a live c0 moved a reload
    // into a sweep). FOLD (references constant over the horizon as well): the backward step's input-row operand r_s = -rho * t + lr_c
    // is not formed; the operator's input columns carry -rho and the accumulator starts carry Mb[:, nx:] * lr_c instead (Step::bwd_fold).
    constexpr bool K0 = !FAM && !ADAPT && !REFILL;
    constexpr bool FOLD = !FAM && !ADAPT && CT && !ITRAJ && !IKBND;

#ifdef TINY_CLOCK_STAMP
    const unsigned long long ck_entry = __builtin_amdgcn_s_memrealtime();
#endif
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int j = lane >> 4, r = lane & 15;
    const long grp = (long)blockIdx.x * WPG + wv;
    const bool grp_ok = grp < p.groups;
    const long inst = grp * IPW + j;
    const bool is_x = r < NX;
    const bool is_u = (r >= NX) && (r < NXU);
    const bool inst_ok = grp_ok && inst < p.batch;
    const int koff = is_x ? 1 : 0;  // slot s = knot s+1 on state lanes, knot s on input lanes

    double *sOps = smem;
#if TINY_LDS_START
    static_assert(!IMOD && !FAM && !ADAPT && !REFILL, "the table of accumulator starts: lean kernels only");
    double *sStart = smem + D_OPS_DOUBLES;  // cf[16 r]
    double *sT = sStart + D_START_DOUBLES;
#else
    double *sT = smem + (IMOD ? 0 : D_OPS_DOUBLES);
#endif
    double *sLin = sT + (CT ? 0 : d_tab_doubles(N));  // FAM
    double *sAd = sLin + (FAM && !ILIN ? D_FAM_DOUBLES : 0);   // ADAPT: [5][16 k][16 r]
#if TINY_TRIM_DSTORE
    static_assert(!IMOD, "the dump rows: lean kernels only");
    double *sV = sAd + (ADAPT ? D_ADAPT_DOUBLES : 0) + (size_t)wv * (VL * 64 + D_DUMP_DOUBLES(NU) + d_d_doubles(NU, N));
    double *sD = sV + VL * 64 + D_DUMP_DOUBLES(NU);  // (rows -1 and -2 of d: written by the dump lanes of the lean backward sweeps, never read)
#else
    double *sV = sAd + (ADAPT ? D_ADAPT_DOUBLES : 0) + (size_t)wv * (VL * 64 + d_d_doubles(NU, N) + (IMOD ? D_IMOD_WAVE_DOUBLES : 0) + d_ilin_wave_doubles(ILIN, IKNOT ? N : 0) +
                                                                       d_itraj_wave_doubles(ITRAJ, N) + d_ikbnd_wave_doubles(IKBND, N));
    double *sD = sV + VL * 64;
#endif
    double *sOpsW = sD + d_d_doubles(NU, N);  // IMOD: [4 instances][D_IMOD_STRIDE]
    double *sLinW = sD + d_d_doubles(NU, N);  // ILIN: [3 nl][64], this wavefront's group of SolveParams::ilin (never together with IMOD); IKNOT: [N slots][3 nl][64]
    // ITRAJ: [N + 2][64], this wavefront's group of SolveParams::iref_lr (never together with IMOD), behind the wavefront's linear rows where the form has both
    double *sRefW = sLinW + d_ilin_wave_doubles(ILIN, IKNOT ? N : 0);
    static_assert(!ITRAJ || sizeof(double) * (D_OPS_DOUBLES + D_START_DOUBLES + VL * 64 + d_d_doubles(NU, N) + d_ilin_wave_doubles(ILIN, IKNOT ? N : 0) + d_itraj_wave_doubles(true, N) +
                                              d_ikbnd_wave_doubles(IKBND, N)) < 65536,
                  "per-instance trajectories: the last row's reads stay below the 16-bit ds offset field, whatever constant part of the address the compiler folds in");
    // IKBND: lo [N + 2][64] | hi [N + 2][64], this wavefront's group of SolveParams::ibnd's two blocks, behind the wavefront's linref rows where the form has both
    double *sBndW = sRefW + d_itraj_wave_doubles(ITRAJ, N);
    constexpr int BHI = (N + 2) * 64;  // (hi lies one block behind lo)
    static_assert(!IKBND || sizeof(double) * (D_OPS_DOUBLES + D_START_DOUBLES + VL * 64 + d_d_doubles(NU, N) + d_itraj_wave_doubles(ITRAJ, N) + d_ikbnd_wave_doubles(true, N)) < 65536,
                  "per-knot bounds: the last row's reads stay below the 16-bit ds offset field, whatever constant part of the address the compiler folds in");
    // (a slot's rows lie LIN_SLOT doubles behind the last slot's: 0 where the rows are constant over the horizon -- one code path)
    constexpr int LIN_SLOT = IKNOT ? 3 * ILIN * 64 : 0;
    static_assert(!IKNOT || sizeof(double) * (D_OPS_DOUBLES + D_START_DOUBLES + VL * 64 + d_d_doubles(NU, N) + d_ilin_wave_doubles(ILIN, N) + d_itraj_wave_doubles(ITRAJ, N)) < 65536,
                  "rows per knot: the last slot's reads stay below the 16-bit ds offset field, whatever constant part of the address the compiler folds in");

    // ---- workgroup-shared: the two sweep operators, transposed to [k][r] (conflict-free row reads), and the tables
    if constexpr (IMOD) {
        // ... per wavefront: the blocks of its four instances, each from the instance's own p.ops block, transposed, padded and scaled
        // like the shared copy (lanes beyond the batch: instance 0's block, as k_admm_solve_imod does)
        if (grp_ok) {
            for (int i = lane; i < IPW * D_OPS_DOUBLES; i += 64) {
                const int jj = i >> 9, e = i & 511, which = e >> 8, k = (e >> 4) & 15, rr = e & 15;
                const long ib = grp * IPW + jj;
                const double *const ops_i = p.ops + (size_t)(ib < p.batch ? ib : 0) * ops_doubles(W, KT);
                const double v = (k < KT) ? ops_i[(size_t)which * W * KT + (size_t)rr * KT + k] : 0.0;
                const double rho_i = ib < p.batch ? p.rho_inst[ib] : p.rho;  // (the block's own instance's rho: tinympc_set_rho_batch)
                sOpsW[jj * D_IMOD_STRIDE + e] = (FOLD && which == 1 && k >= NX) ? -rho_i * v : v;
            }
        }
    } else {
        for (int i = threadIdx.x; i < D_OPS_DOUBLES; i += 64 * WPG) {
            const int which = i >> 8, k = (i >> 4) & 15, rr = i & 15;
            const double v = (k < KT) ? p.ops[(size_t)which * W * KT + (size_t)rr * KT + k] : 0.0;
            sOps[i] = (FOLD && which == 1 && k >= NX) ? -p.rho * v : v;  // (FOLD: -rho * Mb[:, nx:])
        }
    }
#if TINY_LDS_START
    if (threadIdx.x < D_START_DOUBLES) sStart[threadIdx.x] = p.ops[(size_t)2 * W * KT + threadIdx.x];  // cf, as the lanes load it below
#endif
    if constexpr (!CT)
        for (int i = threadIdx.x; i < d_tab_doubles(N); i += 64 * WPG) sT[i] = p.tables[i];
    if constexpr (ADAPT) {  // k_build_adapt's tables: mt | pinf | dpinf | dmf | dmb, each [W][KT]; here: dmf | dmb | mt | pinf | dpinf
        for (int i = threadIdx.x; i < D_ADAPT_DOUBLES; i += 64 * WPG) {
            const int which = i >> 8, k = (i >> 4) & 15, rr = i & 15;
            const int tbl = which == 0 ? 3 : which == 1 ? 4 : which - 2;
            sAd[i] = (k < KT) ? p.adapt[(size_t)tbl * W * KT + (size_t)rr * KT + k] : 0.0;
        }
    }
    if constexpr (ITRAJ) {
        // ... per wavefront: its group's linref rows, verbatim (padding rows, and lanes beyond the batch or the system's rows: zero)
        if (grp_ok) {
            const double *const rows_g = p.iref_lr + (size_t)grp * d_itraj_wave_doubles(true, N);
            for (int i = lane; i < d_itraj_wave_doubles(true, N); i += 64) sRefW[i] = rows_g[i];
        }
    }
    if constexpr (IKBND) {
        // ... per wavefront: its group's clamp rows, lo and hi, verbatim (padding rows, lanes beyond the batch or the system's rows, and a
        // disabled bound family: -inf / +inf)
        if (grp_ok) {
            const double *const lo_g = p.ibnd + (size_t)grp * BHI, *const hi_g = lo_g + (size_t)p.groups * BHI;
            for (int i = lane; i < BHI; i += 64) {
                sBndW[i] = lo_g[i];
                sBndW[BHI + i] = hi_g[i];
            }
        }
    }
    if constexpr (IKNOT) {
        // ... per wavefront: its group's N slots of 3 nl vectors, verbatim -- the slots are in the sweep's skew and the third vector is the
        // reciprocal already (k_build_inst_lin_knots; lanes beyond the batch: a = 0, b = +inf, reciprocal 1 -- the row is off)
        if (grp_ok) {
            const double *const rows_g = p.ilin + (size_t)grp * inst_fam_block_doubles(ILIN, N) + INST_FAM_SLOPE_ROWS * 64;
            for (int i = lane; i < d_ilin_wave_doubles(ILIN, N); i += 64) sLinW[i] = rows_g[i];
        }
    } else if constexpr (ILIN > 0) {
        // ... per wavefront: the 3 nl vectors of its own group, in the kernel's lane order as k_build_inst_lin wrote them (lanes beyond the
        // batch: a = 0, b = +inf, norm 1 -- the row is off); the third vector as its reciprocal, like the shared copy below
        if (grp_ok) {
            const double *const rows_g = p.ilin + (size_t)grp * inst_fam_group_doubles(ILIN) + INST_FAM_SLOPE_ROWS * 64;
            for (int i = lane; i < 3 * ILIN * 64; i += 64) {
                const double v = rows_g[i];
                sLinW[i] = ((i >> 6) % 3 == 2) ? 1.0 / v : v;  // 1 / ||a_k||^2
            }
        }
    } else if constexpr (FAM) {  // layout of fam_doubles(): ... | nl | per linear row k: a_k[W] b_k[W] ||a_k||^2[W]
        const double *lin_rows = p.fam + 4 * W + (size_t)3 * W * KT;
        for (int i = threadIdx.x; i < D_FAM_DOUBLES; i += 64 * WPG) {
            const int k3 = i / W, rr = i % W;
            const double v = lin_rows[1 + (size_t)k3 * W + rr];
            sLin[i] = (k3 % 3 == 2) ? 1.0 / v : v;  // 1 / ||a_k||^2
        }
    }

    const size_t g0 = grp_ok ? (size_t)grp : 0;
    double *const gG = p.G + g0 * (N + 1) * 64 + lane;                 // row kn = knot kn
    double *const gD = p.D + g0 * (size_t)(NS * DS);
    double *const gV0 = p.V + (g0 * v_rows(N) + V_PAD) * 64 + lane;    // canonical v|z, knot 0
#if TINY_REFILL
    // stale copy, knot 0 (wave-uniform: scalar base + 32-bit lane offset; REFILL: the rows of a wavefront belong to different
    // groups of four, so the base is the array's and the offset carries the group -- below 2^32 doubles for any batch that fits HBM)
    double *const gV1u = p.V2 + ((REFILL ? 0 : g0) * v_rows(N) + V_PAD) * 64;
    int cur = (int)inst;  // REFILL: the instance this row works on
    auto row_offset = [&](int i) -> unsigned { return (unsigned)(i >> 2) * (unsigned)(v_rows(N) * 64) + (unsigned)((i & 3) * 16 + r); };
    // (REFILL: rebuilt from `cur` where it is needed -- rare paths -- instead of living in a register across the sweeps)
#else
    double *const gV1u = p.V2 + (g0 * v_rows(N) + V_PAD) * 64;         // stale copy, knot 0 (wave-uniform: scalar base + 32-bit lane offset)
#endif
    const unsigned voff = (unsigned)(lane + koff * 64);
    double *const sVl = sV + lane;
    const bool cold = p.cold != 0;  // (uniform) the state is zero by contract and was never written to HBM: nothing to load
    if (grp_ok) {
        if (cold) {
            for (int i = lane; i < NS * DS; i += 64) sD[i] = 0.0;
            static_for<0, VL>([&](auto S) { sVl[S.value * 64] = 0.0; });
        } else {
            for (int i = lane; i < NS * DS; i += 64) sD[i] = gD[i];
            static_for<0, VL>([&](auto S) { sVl[S.value * 64] = gV0[(S.value + koff) * 64]; });
        }
    }
    __syncthreads();  // the only workgroup-wide barrier: from here on the waves are independent
    if (!grp_ok) return;
#ifdef TINY_CLOCK_STAMP
    const unsigned long long ck_barrier = __builtin_amdgcn_s_memrealtime();
#endif

    // ---- register-resident state
    double G[NS], G0, Vr[NVR > 0 ? NVR : 1], V0;
#if TINY_LEAN_PARK
    // the split inside a run of lean rounds: slots VLR..VL-1 are register slots there (Vx[], live from a run's entry to its last forward sweep)
    static_assert(VL > TINY_PARK_SLOTS && TINY_PARK_SLOTS > 0, "the converted slots are LDS slots, and slot 0 stays one");
    constexpr int VLR = VL - TINY_PARK_SLOTS, NVX = VL - VLR;
    double Vx[NVX];
#endif
    if (cold) {
        static_for<0, NS>([&](auto S) { G[S.value] = 0.0; });
        static_for<0, NVR>([&](auto S) { Vr[S.value] = 0.0; });
        G0 = 0.0;
        V0 = 0.0;
    } else {
        static_for<0, NS>([&](auto S) { G[S.value] = gG[(S.value + koff) * 64]; });
        static_for<0, NVR>([&](auto S) { Vr[S.value] = gV0[(VL + S.value + koff) * 64]; });
        G0 = gG[0];
        V0 = gV0[0];
    }
    // FAM state: slot s <-> knot s + koff, like G / V (the arrays GC / GL have V's shape)
    double GCr[FAM ? NS : 1], GLr[FAM ? NS : 1], LX[FAM ? NS : 1], GC0 = 0.0, GL0 = 0.0;
    double cn[KT], ct_[KT], ty[KT];
    int role = 0, nl = 0;
    double mu = 0.0, inv_mu = 0.0;
    bool famc = false, faml = false, any_cone = false, any_lin = false;
    if constexpr (FAM) {
        const double *const gGC = p.GC + (g0 * v_rows(N) + V_PAD) * 64 + lane, *const gGL = p.GL + (g0 * v_rows(N) + V_PAD) * 64 + lane;
        static_for<0, NS>([&](auto S) {
            GCr[S.value] = gGC[(S.value + koff) * 64];
            GLr[S.value] = gGL[(S.value + koff) * 64];
            LX[S.value] = 0.0;
        });
        GC0 = gGC[0];
        GL0 = gGL[0];
        const double *Cn = p.fam + 4 * W + (size_t)r * KT, *Ct = Cn + (size_t)W * KT, *Ty = Ct + (size_t)W * KT;
#pragma unroll
        for (int k = 0; k < KT; ++k) {
            cn[k] = Cn[k];
            ct_[k] = Ct[k];
            ty[k] = Ty[k];
        }
        role = (int)p.fam[r];
        mu = p.fam[W + r];
        // (ICONE: the lane's INSTANCE's slope, tinympc_set_cone_slopes_batch -- round 0's vector in front of the group's rows in SolveParams::ilin;
        // read once, here: the iteration loop gains no load. The form takes cones without rounds.)
        if constexpr (ICONE) mu = grp_ok ? p.ilin[(size_t)grp * (IKNOT ? inst_fam_block_doubles(ILIN, N) : inst_fam_group_doubles(ILIN)) + lane] : mu;
        inv_mu = (mu != 0.0) ? 1.0 / mu : 0.0;  // (mu = 0: row in no cone)
        famc = p.fam[2 * W + r] != 0.0;
        faml = p.fam[3 * W + r] != 0.0;
        nl = ILIN ? ILIN : (int)p.fam[4 * W + (size_t)3 * W * KT];  // (ILIN: the mode's count, SolveParams::ilin_nl, a constant of the specialisation)
        any_cone = __ballot(famc) != 0ull;  // the same in every 16-lane row
        any_lin = __ballot(faml) != 0ull;
    }
    // One (row, knot) element of the two extra families, exactly as in k_admm_solve_fam / k_admm_solve_c: returns the element's
    // contribution to the linear cost and the new duals. All 16 lanes of the instance take part (no EXEC masking in this kernel).
    // (slot: the knot slot of the call's element in the per-knot form -- 0 for knot 0, q + 1 for forward step q; a constant at every call)
    auto families = [&](double val, double gc_old, double gl_old, double &gc_new, double &gl_new, int slot) -> double {
        const double *const sLinK = sLinW + slot * LIN_SLOT;
        double lxv = 0.0;
        gc_new = gc_old;
        gl_new = gl_old;
        if (any_cone && any_lin && nl == 1) {
            // Both families and a single linear row (the rocket-landing case): the same operations as below, in ONE basic block, so
            // that the scheduler interleaves the three independent mat-vec chains and the two projection sequences -- a lone
            // wavefront issues a dependent FP64 instruction every ~7 cycles, an independent one every ~5.
            const double svc = val + gc_old, s0 = val + gl_old;
            const double a_k = ILIN ? sLinK[lane] : sLin[r], b_k = ILIN ? sLinK[64 + lane] : sLin[W + r], in_k = ILIN ? sLinK[2 * 64 + lane] : sLin[2 * W + r];
            const double a2 = group_matvec<W, KT>(cn, svc * svc, 0.0);
            const double t = group_matvec<W, KT>(ct_, svc, 0.0);
            const double dot = group_matvec<W, KT>(ty, a_k * s0, 0.0);
            const double vc = soc_project_element(svc, a2, t, mu, inv_mu, role);
            const double svl = halfspace_project_element(s0, dot, a_k, b_k, in_k);
            const double gcn = svc - vc, gln = s0 - svl;
            if (famc) {
                gc_new = gcn;
                lxv -= p.rho * (vc - gcn);
            }
            if (faml) {
                gl_new = gln;
                lxv -= p.rho * (svl - gln);
            }
            return lxv;
        }
        if (any_cone) {
            const double sv = val + gc_old;
            const double a2 = group_matvec<W, KT>(cn, sv * sv, 0.0);
            const double t = group_matvec<W, KT>(ct_, sv, 0.0);
            const double vc = soc_project_element(sv, a2, t, mu, inv_mu, role);
            const double gcn = sv - vc;
            if (famc) {
                gc_new = gcn;
                lxv -= p.rho * (vc - gcn);
            }
        }
        if (any_lin) {
            const double s0 = val + gl_old;
            double sv = s0;
#pragma unroll 1
            for (int k = 0; k < nl; ++k) {  // (uniform trip count)
                const double a_k = ILIN ? sLinK[(3 * k + 0) * 64 + lane] : sLin[(3 * k + 0) * W + r];
                const double b_k = ILIN ? sLinK[(3 * k + 1) * 64 + lane] : sLin[(3 * k + 1) * W + r];
                const double in_k = ILIN ? sLinK[(3 * k + 2) * 64 + lane] : sLin[(3 * k + 2) * W + r];
                const double dot = group_matvec<W, KT>(ty, a_k * sv, 0.0);
                sv = halfspace_project_element(sv, dot, a_k, b_k, in_k);
            }
            const double gln = s0 - sv;
            if (faml) {
                gl_new = gln;
                lxv -= p.rho * (sv - gln);
            }
        }
        return lxv;
    };
    const bool row_ok = r < NXU;

    // (IMOD: from this lane's instance's block of p.ops, at opsI; otherwise the one shared block, in the expressions it always had -- as one
    // pointer for both forms the plain kernels kept their instructions but not their order)
    size_t opsI = 0;  // (doubles)
    if constexpr (IMOD) opsI = (size_t)(inst_ok ? inst : 0) * ops_doubles(W, KT);
    const double cf = IMOD ? p.ops[opsI + (size_t)2 * W * KT + r] : p.ops[(size_t)2 * W * KT + r];
    const double cb = IMOD ? p.ops[opsI + (size_t)2 * W * KT + W + r] : p.ops[(size_t)2 * W * KT + W + r];
    const double pnref0 = IGOAL ? (inst_ok ? p.iref_pn[inst * W + r] : 0.0) : p.tables[(size_t)3 * TOFF + r];
    // (ADAPT: rho, its negative and pNref are lane variables that change every fifth iteration; otherwise they never change and
    // stay in scalar registers)
    const double rho0 = p.rho;
    double rho = p.rho, pnref = pnref0;
    double dpnref = 0.0, dgr = 0.0;
    if constexpr (ADAPT) {
        rho = inst_ok ? p.rho_inst[inst] : rho0;  // persists across solves like cache->rho
        dpnref = p.adapt[(size_t)5 * W * KT + r];
        dgr = p.ops[(size_t)2 * W * KT + 2 * W + r];  // Q + rho0 / R + rho0 diagonal of this row (tiny_api.cpp:90-91)
        pnref = fma(rho - rho0, dpnref, pnref0);
    }
    // IMOD: the instance's own rho (tinympc_set_rho_batch; the handle's where the verb never named it) -- a lane variable, constant over the solve
    if constexpr (IMOD) rho = inst_ok ? p.rho_inst[inst] : rho0;
    double nrho = -rho;
    // (IKBND: ibnd is the store of every knot's rows, not [instance][16] -- the form reads its clamps from sBndW and has no lo_c / hi_c)
#if TINY_REFILL
    // (REFILL with IGOAL: the four lane constants belong to the row's CURRENT instance -- reloaded where the row takes its next one)
    double lo_c = IKBND ? 0.0 : IGOAL ? (inst_ok ? p.ibnd[inst * W + r] : 0.0) : p.tables[W + r];
    double hi_c = IKBND ? 0.0 : IGOAL ? (inst_ok ? p.ibnd[(size_t)p.groups * 64 + inst * W + r] : 0.0) : p.tables[(size_t)TOFF + W + r];
    double lr_c = ITRAJ ? 0.0 : IGOAL ? (inst_ok ? p.iref_lr[inst * W + r] : 0.0) : p.tables[(size_t)2 * TOFF + W + r];
#else
    const double lo_c = IKBND ? 0.0 : IGOAL ? (inst_ok ? p.ibnd[inst * W + r] : 0.0) : p.tables[W + r];
    const double hi_c = IKBND ? 0.0 : IGOAL ? (inst_ok ? p.ibnd[(size_t)p.groups * 64 + inst * W + r] : 0.0) : p.tables[(size_t)TOFF + W + r];
    // (ITRAJ: iref_lr is the store of every knot's rows, not [instance][16] -- the form reads its linref from sRefW and has no lr_c)
    const double lr_c = ITRAJ ? 0.0 : IGOAL ? (inst_ok ? p.iref_lr[inst * W + r] : 0.0) : p.tables[(size_t)2 * TOFF + W + r];
#endif
    double rhom = is_x ? nrho : 0.0;
#if TINY_REFILL
    double x0v = (inst_ok && is_x) ? p.x0[inst * NX + r] : 0.0;
#else
    const double x0v = (inst_ok && is_x) ? p.x0[inst * NX + r] : 0.0;
#endif
    if constexpr (HOSTX) {  // zero-copy tick: x0 came from pinned host memory
        if (p.x0_mirror && inst_ok && is_x) p.x0_mirror[inst * NX + r] = x0v;
    }
    const int dIdx = j * NU + (is_u ? r - NX : 0);
    const double *const sDr = sD + dIdx;
    double *const sDw = sD + dIdx;
    const double *const sTl = sT + koff * W + r;  // (!CT) row of slot s: sTl[(s + 1) * W]
    const double *const sMf = (IMOD ? sOpsW + j * D_IMOD_STRIDE : sOps) + r, *const sMb = sMf + 256;
    const unsigned aV = lds_addr(sVl), aD = lds_addr(sDr), aT = lds_addr(sTl);
    const unsigned aR = ITRAJ ? lds_addr(sRefW + koff * 64 + lane) : 0u;  // (ITRAJ) row of slot s: offset (s + 1) * 512 -- the knot the shared table's sTl reads
    const unsigned aB = IKBND ? lds_addr(sBndW + koff * 64 + lane) : 0u;  // (IKBND) lo of slot s: offset (s + 1) * 512, hi BHI * 8 behind it
#if TINY_LDS_START
    const unsigned aC = lds_addr(sStart + r);
#endif
    const int ct = p.check_termination;
    // K0: c0 = cf + Mf[:, :nx] * x_0 -- the chain's state columns, its FMAs in its order, so forward step 0 (the input columns behind
    // c0) is bit-identical to the full chain.
    double c0 = 0.0;
    if constexpr (K0) {
        c0 = cf;
        static_for<0, NX>([&](auto K) { c0 = fma(__shfl(x0v, (lane & 48) + K.value), sMf[K.value * 16], c0); });
    }
    // FOLD: the accumulator start of a backward step, lr_c + cb on state lanes and cb on input lanes, plus Mb[:, nx:] * lr_c (the input
    // lanes' lr_c, the unscaled operator); the same expression in the shared-table and the per-instance goal kernels
    double lrmc_f = 0.0;
    if constexpr (FOLD) {
        double mb[16];
        static_for<0, 16>([&](auto K) { mb[K.value] = (K.value >= NX && K.value < NXU) ? p.ops[(size_t)W * KT + (size_t)r * KT + K.value] : 0.0; });
        if constexpr (IMOD) static_for<NX, NXU>([&](auto K) { mb[K.value] = p.ops[opsI + (size_t)W * KT + (size_t)r * KT + K.value]; });
        lrmc_f = Step::acc_inputs(is_x ? lr_c + cb : cb, lr_c, mb);
    }

    // Control: an instance that converges stops being `active` but its lanes keep iterating as a zombie (the sweeps are
    // unconditional for all 64 lanes -- no EXEC-masked region around the unrolled body). Its state is written back at
    // the top of the next round, before the next forward sweep touches G and V; the backward sweep in between leaves
    // G and V alone and skips a zombie's d. Instances that hit max_iter are written back by the same code in round
    // `max_iter`, which does nothing else.
    bool active = inst_ok;
    bool pending = false;  // converged in the previous round: state not yet written back
    int it_done = 0;
    int status = 11;  // TINY_UNSOLVED (admm.cpp:114)
    bool res_valid = false;
    double snap_pri = 0.0, snap_dua = 0.0, snap_rho = p.rho;

    auto load_ops = [&](const double *src, double (&m)[16]) {  // (src: sMf / sMb; ADAPT: the derivative rows sit 512 doubles behind)
        if constexpr (ADAPT) {
            const double delta = rho - rho0;
            static_for<0, 16>([&](auto K) {
                constexpr int o = (K.value < NXU ? K.value : 0) * 16;
                m[K.value] = fma(delta, src[o + (sAd - sOps)], src[o]);
            });
        } else {
            static_for<0, 16>([&](auto K) { m[K.value] = src[(K.value < NXU ? K.value : 0) * 16]; });
        }
    };
    auto vget = [&](auto S) -> double {
        if constexpr (decltype(S)::value >= VL) return Vr[decltype(S)::value - VL];
        else return sVl[decltype(S)::value * 64];
    };

#ifdef TINY_CLOCK_STAMP  // diagnostic build only (tools/clock_check.py): the shader clock held under this kernel
    const unsigned long long ck_t0 = __builtin_amdgcn_s_memtime(), ck_r0 = __builtin_amdgcn_s_memrealtime();
#endif
#ifdef TINY_D_PAD  // (experiment: TINY_D_PAD s_nop in front of the iteration loop -- shifts the loop's code by 4 bytes each)
    asm volatile(".rept " TINY_STR(TINY_D_PAD) "\n\ts_nop 0\n\t.endr" ::: "memory");
#endif
#ifdef TINY_D_LOOP_ALIGN  // (experiment: the iteration loop's code starts on a 2^TINY_D_LOOP_ALIGN byte boundary)
    asm volatile(".p2align " TINY_STR(TINY_D_LOOP_ALIGN) ::: "memory");
#endif
    const int max_iter = p.max_iter;
#if TINY_TRIM_DSTORE
    unsigned aDw = aD;  // where this lane's d stores of a lean round go: set in front of every run of lean rounds
#endif
#if TINY_LEAN_PARK
    // What lives across a run of lean rounds without being used in it goes to LDS at the run's entry and comes back in the run's last
    // round, between its forward sweep (behind which Vx[] is dead) and its backward sweep: the registers are free inside the run. The
    // place is the rows VLR..NS-1 of the wavefront's d, taken as [PARK_ROWS][64 lanes]: the entry has just read them into Vr[] / Vx[],
    // no shared round reads or writes them (register slots; the dump rows of the blocks that still store lie below VLR - 1), and the
    // last round's backward sweep, which rewrites them for every live instance, comes behind the reload. (Instances that are not live
    // keep the parked bits in those rows: their write-back is done, and nothing reads what their lanes compute from them.)
    constexpr int PARK_ROWS = 3;
    static_assert(PARK_ROWS * 64 <= (NS - VLR) * DS, "the parked rows fit into the d rows of the run's register slots");
    auto park = [&]() __attribute__((always_inline)) {
        const unsigned aP = lds_addr(sD + VLR * DS + lane);
        lds_write_async<0 * 512>(aP, snap_pri);
        lds_write_async<1 * 512>(aP, snap_dua);
        lds_write_async<2 * 512>(aP, __hiloint2double(status, it_done));
    };
    auto unpark = [&]() __attribute__((always_inline)) {
        const unsigned aP = lds_addr(sD + VLR * DS + lane);
        double p0 = lds_read_async<0 * 512>(aP), p1 = lds_read_async<1 * 512>(aP), p2 = lds_read_async<2 * 512>(aP);
        lds_wait();
        asm volatile("" : "+v"(p0), "+v"(p1), "+v"(p2));  // (the reads are consumed behind their wait)
        snap_pri = p0;
        snap_dua = p1;
        status = __double2hiint(p2);
        it_done = __double2loint(p2);
    };
#endif
#if TINY_LEAN
    // One round of the loop below, in two forms: LEAN_ = true without residuals, false the plain kernel's. Returns true when the solve
    // is over. (Each form is called from one place and inlined there.)
    auto iteration = [&](auto LEAN_, const int it) __attribute__((always_inline)) -> bool {
#if TINY_LEAN_HOIST
        // (2: the control of a run of lean rounds alone -- write-back of what the last iteration with residuals left pending, then
        // "is anything still iterating"; the lean rounds proper, 1, have neither)
        constexpr bool LEANI = decltype(LEAN_)::value != 0, CTL_ONLY = decltype(LEAN_)::value == 2, NO_CTL = LEANI && !CTL_ONLY;
#if TINY_LEAN_SHARE
        // (3: the shared round -- forward AND backward sweep on the shared registers; 4: the last round of a run -- the shared forward
        // sweep with the unshared backward sweep; see TINY_LEAN_SHARE at the top of the file. The unshared lean round, 1, is not used.)
        constexpr bool SH_F = decltype(LEAN_)::value >= 3, SH_B = decltype(LEAN_)::value == 3;
#endif
#else
        constexpr bool LEANI = decltype(LEAN_)::value;
#endif
#else
    for (int it = 0; max_iter > 0; ++it) {  // admm.cpp:129
#endif
        // (readfirstlane: keeps the loop counter and everything derived from it in SGPRs, so that the branches below
        // are scalar branches and not EXEC-masked regions)
        const int it0 = __builtin_amdgcn_readfirstlane(it);
#if TINY_LEAN
        const bool final_round = !LEANI && it0 >= max_iter;  // (a lean round is never the last: see the loop behind this lambda)
#elif TINY_REFILL
        const bool final_round = REFILL ? false : it0 >= max_iter;  // (REFILL: every row has its own count, `fin` below)
#else
        const bool final_round = it0 >= max_iter;
#endif
#if TINY_LEAN_HOIST
        if constexpr (TWO_PER_SIMD && !CTL_ONLY) fair_share_priority<NS>(it0, simd_slot);
#else
        if constexpr (TWO_PER_SIMD) fair_share_priority<NS>(it0, simd_slot);  // (tinympc_sweep.h: the two wavefronts of a SIMD finish together)
#endif
        // ---- write-back: G, D and the canonical v|z (not converged: v = vnew, admm.cpp:196-197; converged: the solve
        // returned before v <- vnew, so the canonical copy is the stale one in V2); solution = vnew / znew (:187-188, 204-205)
#if TINY_REFILL
        const bool fin = REFILL ? it_done >= max_iter : final_round;
        const bool wb = pending || (fin && active);
#elif TINY_LEAN_HOIST
        const bool wb = NO_CTL ? false : pending || (final_round && active);  // (a lean round: the block below folds away)
#else
        const bool wb = pending || (final_round && active);
#endif
        if (TINY_RARE(__ballot(wb) != 0ull)) {
            // Rare path (once per instance and solve), kept small in registers rather than fast: addresses are rebuilt
            // here from the kernel arguments (the opaque copy of `lane` keeps the compiler from hoisting them out of
            // the iteration loop, where they would occupy registers the unrolled sweeps need).
            int lane_o = lane;
            asm volatile("" : "+v"(lane_o));
            const int r_o = lane_o & 15, j_o = lane_o >> 4;
            const bool x_o = r_o < NX;
#if TINY_REFILL
            // (REFILL: this row's instance; its place in the group-of-four layout of the state arrays)
            int cur_o = cur;
            if constexpr (REFILL) asm volatile("" : "+v"(cur_o));
            const size_t grp_w = REFILL ? (size_t)(cur_o >> 2) : (size_t)grp;
            const int lane_w = REFILL ? (cur_o & 3) * 16 + r_o : lane_o;
#endif
            if (wb && r_o < NXU) {
                const int ko = x_o ? 1 : 0;
#if TINY_REFILL
                const size_t inst_o = REFILL ? (size_t)cur_o : (size_t)grp * IPW + j_o;
                double *const wG = p.G + grp_w * (N + 1) * 64 + lane_w + ko * 64;                // slot 0
                double *const wV = p.V + (grp_w * v_rows(N) + V_PAD) * 64 + lane_w + ko * 64;   // slot 0
#else
                const size_t inst_o = (size_t)grp * IPW + j_o;
                double *const wG = p.G + (size_t)grp * (N + 1) * 64 + lane_o + ko * 64;                // slot 0
                double *const wV = p.V + ((size_t)grp * v_rows(N) + V_PAD) * 64 + lane_o + ko * 64;   // slot 0
#endif
                double *const wS = x_o ? p.sol_x + (inst_o * N + 1) * NX + r_o : p.sol_u + inst_o * NS * NU + (r_o - NX);  // slot 0
                const int sst = x_o ? NX : NU;
                if (x_o) {  // knot 0
                    wG[-64] = G0;
                    wV[-64] = V0;
                    wS[-NX] = V0;
                }
                static_for<0, NS>([&](auto S) {
                    constexpr int s = decltype(S)::value;
                    const double vn = vget(S);
                    wG[s * 64] = G[s];
                    wV[s * 64] = vn;
                    wS[s * sst] = vn;
                    if constexpr (HOSTX && s == 0) {  // zero-copy tick: the first controls also go straight into pinned host memory
                        if (p.u0_host && !x_o) p.u0_host[inst_o * NU + (r_o - NX)] = vn;
                    }
                });
                if constexpr (FAM) {
                    double *const wGC = p.GC + ((size_t)grp * v_rows(N) + V_PAD) * 64 + lane_o + ko * 64;
                    double *const wGL = p.GL + ((size_t)grp * v_rows(N) + V_PAD) * 64 + lane_o + ko * 64;
                    static_for<0, NS>([&](auto S) {
                        wGC[S.value * 64] = GCr[S.value];
                        wGL[S.value * 64] = GLr[S.value];
                    });
                    if (x_o) {
                        wGC[-64] = GC0;
                        wGL[-64] = GL0;
                    }
                }
                if (!x_o) {
#if TINY_REFILL
                    double *const wD = p.D + grp_w * (NS * DS) + (REFILL ? (cur_o & 3) : j_o) * NU + (r_o - NX);
#else
                    double *const wD = p.D + (size_t)grp * (NS * DS) + j_o * NU + (r_o - NX);
#endif
                    for (int i = 0; i < NS; ++i) wD[i * DS] = sDw[i * DS];
#if TINY_REFILL
                }
            }
            if constexpr (REFILL) {
                // ---- what the plain kernel does behind its loop, here for the rows that are being written back
                // A converged solve returned before v <- vnew (admm.cpp:181-197): its canonical v|z is the stale copy.
                if (wb && status == 1 && r_o < NXU) {
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    const int rows = x_o ? N : NS;
                    double *const cV = p.V + (grp_w * v_rows(N) + V_PAD) * 64 + lane_w;
                    const double *const cV2 = p.V2 + (grp_w * v_rows(N) + V_PAD) * 64 + lane_w;
                    for (int kn = 0; kn < rows; ++kn) cV[kn * 64] = cV2[kn * 64];
                }
                const double s_px = group_max<W>(is_x ? snap_pri : 0.0), s_pu = group_max<W>(is_u ? snap_pri : 0.0);
                const double s_dx = group_max<W>(is_x ? snap_dua : 0.0) * rho, s_du = group_max<W>(is_u ? snap_dua : 0.0) * rho;
                if (wb && r_o == 0) {
                    p.istats[(size_t)cur_o * 2 + 0] = it_done;
                    p.istats[(size_t)cur_o * 2 + 1] = status;
                    if (res_valid) {
                        p.dstats[(size_t)cur_o * 4 + 0] = s_px;
                        p.dstats[(size_t)cur_o * 4 + 1] = s_dx;
                        p.dstats[(size_t)cur_o * 4 + 2] = s_pu;
                        p.dstats[(size_t)cur_o * 4 + 3] = s_du;
                    }
                }
                // ---- the next instance of the batch for this row (or none: the row idles as a zombie until the wavefront is done)
                int nxt = 0x7fffffff;
                if (wb && r_o == 0) nxt = (int)(gridDim.x * WPG * IPW) + atomicAdd(p.refill_next, 1);
                nxt = __shfl(nxt, lane_o & 48);
                const bool take = wb && nxt < p.batch;
                if (wb) {
                    active = take;
                    status = 11;
                    res_valid = false;
                    snap_pri = 0.0;
                    snap_dua = 0.0;
                    it_done = 0;
                }
                if (__ballot(take) != 0ull) {
                    if (take) cur = nxt;
                    const size_t grp_n = (size_t)(nxt >> 2);
                    const int lane_n = (nxt & 3) * 16 + r_o;
                    if (take && x_o) x0v = p.x0[(size_t)nxt * NX + r_o];
                    if constexpr (IGOAL) {
                        // The goal form: the taking rows' lane constants are their new instance's ([instance][16]; ibnd's hi half at
                        // groups * 64), and so is the folded accumulator start -- the kernel start's expression on the same operands.
                        // Its chain exchanges values across the 16-lane row: executed by every lane, then selected on `take` (whole rows).
                        // (ITRAJ / IKBND: the constants the form loads per instance at kernel start -- it has no lr_c with trajectories, no
                        // lo_c / hi_c with bounds per knot -- and no folded start: FOLD is off, every backward block forms its own from the row it reads)
                        static_assert(!IMOD && ILIN == 0 && FOLD == (!ITRAJ && !IKBND), "slot refill: the goal form of the box path, its trajectory and per-knot bounds forms");
                        if (take) {
                            const size_t io = (size_t)nxt * W + r_o;
                            if constexpr (!ITRAJ) lr_c = p.iref_lr[io];
                            pnref = p.iref_pn[io];
                            if constexpr (!IKBND) {
                                lo_c = p.ibnd[io];
                                hi_c = p.ibnd[(size_t)p.groups * 64 + io];
                            }
                        }
                        if constexpr (FOLD) {
                            double mb[16];
                            static_for<0, 16>([&](auto K) { mb[K.value] = (K.value >= NX && K.value < NXU) ? p.ops[(size_t)W * KT + (size_t)r_o * KT + K.value] : 0.0; });
                            const double lrmc_n = Step::acc_inputs(x_o ? lr_c + cb : cb, lr_c, mb);
                            lrmc_f = take ? lrmc_n : lrmc_f;
                        }
                        if constexpr (ITRAJ || IKBND) {
                            // The rows the wavefront staged at kernel start are its FIRST group's. A taking row restages its own 16-lane column of
                            // them -- (lane & 48) + r, every row, padding rows and lanes beyond the system's rows included -- from its new
                            // instance's column, (nxt & 3) * 16 + r of group nxt >> 2's block; the other three rows' columns are not touched (their
                            // instances generally belong to other groups). The region is this wavefront's own: no barrier. The take path stands at
                            // the iteration boundary -- every read the backward sweep issued a block ahead was consumed behind its block's wait --,
                            // and the sweeps' reads of these rows (volatile, issued a block ahead) are kept behind the stores by the wait below.
                            auto restage = [&](double *dst, const double *src) {
                                double *const d = dst + lane_o;
                                const double *const g = src + grp_n * (size_t)BHI + lane_n;
#pragma unroll 4
                                for (int k = 0; k < N + 2; ++k) d[k * 64] = g[k * 64];
                            };
                            if (take) {
                                if constexpr (ITRAJ) restage(sRefW, p.iref_lr);
                                if constexpr (IKBND) {
                                    restage(sBndW, p.ibnd);
                                    restage(sBndW + BHI, p.ibnd + (size_t)p.groups * BHI);  // (hi: one array of blocks behind lo, as the kernel start reads it)
                                }
                            }
                            lds_wait();  // (lgkmcnt(0) and a compiler barrier: the stores have retired before the next sweep's first read is issued)
                        }
                    }
                    if (cold) {
                        static_for<0, NS>([&](auto S) { G[S.value] = take ? 0.0 : G[S.value]; });
                        static_for<0, NVR>([&](auto S) { Vr[S.value] = take ? 0.0 : Vr[S.value]; });
                        G0 = take ? 0.0 : G0;
                        V0 = take ? 0.0 : V0;
                        if (take) {
                            static_for<0, VL>([&](auto S) { sVl[S.value * 64] = 0.0; });
                            if (!x_o && r_o < NXU)
                                for (int i = 0; i < NS; ++i) sDw[i * DS] = 0.0;
                        }
                    } else if (take) {
                        const double *const nG = p.G + grp_n * (N + 1) * 64 + lane_n;
                        const double *const nV = p.V + (grp_n * v_rows(N) + V_PAD) * 64 + lane_n;
                        static_for<0, NS>([&](auto S) { G[S.value] = nG[(S.value + koff) * 64]; });
                        static_for<0, NVR>([&](auto S) { Vr[S.value] = nV[(VL + S.value + koff) * 64]; });
                        static_for<0, VL>([&](auto S) { sVl[S.value * 64] = nV[(S.value + koff) * 64]; });
                        G0 = nG[0];
                        V0 = nV[0];
                        if (!x_o && r_o < NXU) {
                            const double *const nD = p.D + grp_n * (NS * DS) + (nxt & 3) * NU + (r_o - NX);
                            for (int i = 0; i < NS; ++i) sDw[i * DS] = nD[i * DS];
                        }
                    }
#endif
                }
            }
            pending = false;
        }
#if TINY_LEAN_HOIST
        if constexpr (!NO_CTL) {
            if (final_round || __ballot(active) == 0ull) return true;
        }
        if constexpr (CTL_ONLY) return false;
#elif TINY_LEAN
        if (final_round || __ballot(active) == 0ull) return true;
#else
        if (final_round || __ballot(active) == 0ull) break;
#endif
        const int it1 = it0 + 1;
#if TINY_LEAN
        // (a lean round: no check falls on it, or none that anything can read)
        const bool check = !LEANI && __builtin_amdgcn_readfirstlane((int)((ct > 0) && ((it1 % ct) == 0))) != 0;
#elif TINY_REFILL
        // admm.cpp:91 (iter already incremented, :143). REFILL: every row checks by its own count; `check` = some live row does.
        bool chk = true, check_r = false;
        if constexpr (REFILL) {
            chk = active && (ct > 0) && (((it_done + 1) % ct) == 0);
            check_r = __ballot(chk) != 0ull;
        }
#define TINY_CHECK_PLAIN (__builtin_amdgcn_readfirstlane((int)((ct > 0) && ((it1 % ct) == 0))) != 0)
        const bool check = REFILL ? check_r : TINY_CHECK_PLAIN;
#undef TINY_CHECK_PLAIN
#else
        const bool check = __builtin_amdgcn_readfirstlane((int)((ct > 0) && ((it1 % ct) == 0))) != 0;  // admm.cpp:91 (iter already incremented, :143)
#endif

        double pri = 0.0, dua = 0.0;
        bool may = check;  // wave-uniform: can this sweep still end converged for some instance of the wave?
        double m[16];
        load_ops(sMf, m);
        // ADAPT: every fifth iteration (admm.cpp:155) the norms of the reference's KKT residuals ride on the forward sweep
        const bool adapt = ADAPT && __builtin_amdgcn_readfirstlane((int)((it0 > 0) && (it0 % 5 == 0))) != 0;
        double a_pr = 0.0, a_pn = 0.0, a_dr = 0.0, a_dn = 0.0;  // primal residual / norm, dual residual / norm
        double gprev = 0.0;  // g_i of the state rows; the x_0 column has no -g_0 term (y_vector starts at g_1)
        double mtr[16];      // this lane's row of [A'; B']
        if constexpr (ADAPT) {
            if (adapt) static_for<0, 16>([&](auto K) { mtr[K.value] = K.value < NXU ? sAd[2 * 256 + K.value * 16 + r] : 0.0; });
        }
        // ---------------- knot 0, state lanes: x_0 is given (tiny_set_x0), no mat-vec
        {
            double lo0, hi0;  // (IKBND: knot 0's row of the wavefront's own block, row 1 -- on every lane, like the shared table's)
            if constexpr (IKBND) {
                lo0 = sBndW[64 + lane];
                hi0 = sBndW[BHI + 64 + lane];
            } else {
                lo0 = CT ? lo_c : sT[W + r];
                hi0 = CT ? hi_c : sT[TOFF + W + r];
            }
            const double s = x0v + G0;
            const double snew = fmin(hi0, fmax(lo0, s));
#if TINY_LEAN_HOIST
            if constexpr (LEANI) G0 = s;  // (G0 = s - snew follows in front of the backward sweep's first block, see there)
            else G0 = s - snew;
#else
            G0 = s - snew;
#endif
            pri = is_x ? fabs(x0v - snew) : 0.0;
            dua = is_x ? fabs(V0 - snew) : 0.0;
            // First "can this sweep still converge" test, on knot 0's residuals alone (exact like the later ones: the
            // maxima only grow). With tolerances nothing can meet -- forced iteration counts -- the sweep writes no stale copy.
            if (may && !adapt) {
                const bool bad = !((pri < p.abs_pri_tol) && (dua * rho < p.abs_dua_tol));
#if TINY_REFILL
                may = __builtin_amdgcn_readfirstlane((int)wave_may_converge_d(__ballot(bad), __ballot(REFILL ? chk : active))) != 0;
#elif TINY_LEAN_PARK
                // (the test on 32-bit halves: the 64-bit form keeps two 64-bit constants in vector registers across the run)
                may = __builtin_amdgcn_readfirstlane((int)wave_may_converge_d32(__ballot(bad), __ballot(active))) != 0;
#else
                may = __builtin_amdgcn_readfirstlane((int)((ILIN || ITRAJ || IKBND) ? wave_may_converge_d32(__ballot(bad), __ballot(active)) : wave_may_converge_d(__ballot(bad), __ballot(active)))) != 0;
#endif
            }
#if TINY_REFILL
            if (TINY_RARE(may) && is_x && active) gV1u[REFILL ? row_offset(cur) : (unsigned)lane] = V0;
#elif TINY_LEAN_PARK
            if (TINY_RARE(may) && is_x && active) {  // (as below, the address built in the rare path: no 64-bit pointer lives across the run)
                unsigned lo = (unsigned)lane;
                double *base = gV1u;
                asm volatile("" : "+v"(lo), "+s"(base));
                base[lo] = V0;
            }
#else
            if (TINY_RARE(may) && is_x && active) gV1u[(unsigned)lane] = V0;  // (active: see the stale copy of the slots below)
#endif
            V0 = snew;
        }
        if constexpr (FAM) {  // knot 0 of the state rows (its lx only reaches p_0, which nothing reads; the duals persist)
            double gcn, gln;
            (void)families(x0v, GC0, GL0, gcn, gln, 0);
            if (is_x) {
                GC0 = gcn;
                GL0 = gln;
            }
        }
        // ---------------- forward sweep (F1) with S1 + D1 + R1 fused in
        // LDS operands of a step (its d, and vold of its slot if that lives in LDS) are requested right before the
        // PREVIOUS step's block and retired by the wait behind that block (lds_reads_landed, inside the Step functions).
        double xcur = x0v;
#if TINY_LEAN_PARK
        // (as below; slot 0 is an LDS slot inside a run too)
        double dcur = lds_read_async<0>(aD), vcur = 0.0;
#elif TINY_LEAN_SHARE
        // (a shared step of a register slot has its d in the slot's register: no read is issued for it)
        double dcur = 0.0, vcur = 0.0;
        if constexpr (!(SH_F && VL == 0)) dcur = lds_read_async<0>(aD);
#else
        double dcur = lds_read_async<0>(aD), vcur = 0.0;
#endif
#if TINY_LEAN
        // (a lean step does not read vold: the read is not issued -- an issued asynchronous read must be consumed behind its wait)
        if constexpr (VL > 0 && !LEANI) vcur = lds_read_async<0>(aV);
#else
        if constexpr (VL > 0) vcur = lds_read_async<0>(aV);
#endif
        // (!CT: bounds that vary over the horizon come from the workgroup's LDS copy of the tables, one step ahead like d)
        double locur = lo_c, hicur = hi_c;
        if constexpr (IKBND) {  // (... or from the wavefront's own clamp rows, the same way)
            locur = lds_read_async<512>(aB);
            hicur = lds_read_async<(BHI + 64) * 8>(aB);
        } else if constexpr (!CT) {
            locur = lds_read_async<W * 8>(aT);
            hicur = lds_read_async<(TOFF + W) * 8>(aT);
        }
        lds_wait_ops(m);
#if TINY_LDS_START
        double acur = 0.0;  // the accumulator of the step at hand, holding its start value (lean sweeps, from step 1 on)
#endif
        auto fstep = [&](auto S) {
            constexpr int q = decltype(S)::value;
            double dn = 0.0, vn = 0.0, lon = lo_c, hin = hi_c;
#if TINY_LEAN_PARK
            // (the register slots of a run start at VLR: no d read from there on)
            if constexpr (q + 1 < NS && !(SH_F && q + 1 >= VLR)) dn = lds_read_async<(q + 1) * DS * 8>(aD);
#elif TINY_LEAN_SHARE
            if constexpr (q + 1 < NS && !(SH_F && q + 1 >= VL)) dn = lds_read_async<(q + 1) * DS * 8>(aD);
#else
            if constexpr (q + 1 < NS) dn = lds_read_async<(q + 1) * DS * 8>(aD);
#endif
#if TINY_LEAN
            if constexpr (q + 1 < VL && !LEANI) vn = lds_read_async<(q + 1) * 512>(aV);
#else
            if constexpr (q + 1 < VL) vn = lds_read_async<(q + 1) * 512>(aV);
#endif
            if constexpr (IKBND) {  // (nested: a condition that depends on the step would capture aB in every form's lambda)
                if constexpr (q + 1 < NS) {
                    lon = lds_read_async<(q + 2) * 512>(aB);
                    hin = lds_read_async<(BHI + (q + 2) * 64) * 8>(aB);
                }
            } else if constexpr (!CT && q + 1 < NS) {
                lon = lds_read_async<(q + 2) * W * 8>(aT);
                hin = lds_read_async<(TOFF + (q + 2) * W) * 8>(aT);
            }
#if TINY_LDS_START
            // (the NEXT step's accumulator start, cf: in flight during this step's block like d_{q+1}; step 0 starts from c0)
            static_assert(K0, "step 0 starts from c0");
            double an = 0.0;
            if constexpr (LEANI && q + 1 < NS) an = lds_read_issued_here<0>(aC);
#endif
            const double xprev = xcur;
            double snew_q;
#if TINY_LEAN
            if constexpr (LEANI) {  // S1 + D1 without R1's maxima: the clamp goes straight into the slot
#if TINY_LEAN_PARK
                if constexpr (SH_F && q >= VLR && q < VL) {
                    // A converted slot: its d is in Vx[q-VLR]. In a shared round that register takes the clamp (the register-slot text); in
                    // the last round of a run the clamp goes to the slot's LDS row, where the backward sweep on VL reads it.
                    if constexpr (SH_B) {
                        xcur = Step::fwd_reg_start(xcur, Vx[q - VLR], m, acur, locur, hicur, G[q], Vx[q - VLR]);
                        snew_q = Vx[q - VLR];
                    } else {
                        double vnew;
                        xcur = Step::fwd_lds_start(xcur, Vx[q - VLR], m, acur, locur, hicur, G[q], vnew);
                        lds_write_async<q * 512>(aV, vnew);
                        snew_q = vnew;
                    }
                } else
#endif
                if constexpr (q >= VL) {
#if TINY_LEAN_SHARE
                    // (shared: the slot's register is the d operand and takes the clamp behind the chain's last read of it)
                    if constexpr (SH_F && K0 && q == 0) xcur = Step::fwd_reg0_nores(Vr[q - VL], m, c0, locur, hicur, G[q], Vr[q - VL]);
                    else if constexpr (SH_F) xcur = Step::fwd_reg_start(xcur, Vr[q - VL], m, acur, locur, hicur, G[q], Vr[q - VL]);
                    else
#endif
                    if constexpr (K0 && q == 0) xcur = Step::fwd_reg0_nores(dcur, m, c0, locur, hicur, G[q], Vr[q - VL]);
#if TINY_LDS_START
                    else xcur = Step::fwd_reg_start(xcur, dcur, m, acur, locur, hicur, G[q], Vr[q - VL]);
#else
                    else xcur = Step::fwd_reg_nores(xcur, dcur, m, cf, locur, hicur, G[q], Vr[q - VL]);
#endif
                    snew_q = Vr[q - VL];
                } else {
                    double vnew;
                    if constexpr (K0 && q == 0) xcur = Step::fwd_lds0_nores(dcur, m, c0, locur, hicur, G[q], vnew);
#if TINY_LDS_START
                    else xcur = Step::fwd_lds_start(xcur, dcur, m, acur, locur, hicur, G[q], vnew);
#else
                    else xcur = Step::fwd_lds_nores(xcur, dcur, m, cf, locur, hicur, G[q], vnew);
#endif
                    lds_write_async<q * 512>(aV, vnew);
                    snew_q = vnew;
                }
            } else
#endif
            if constexpr (q >= VL) {
                if constexpr (K0 && q == 0) xcur = Step::fwd_reg0(dcur, m, c0, locur, hicur, G[q], Vr[q - VL], pri, dua);
                else xcur = Step::fwd_reg(xcur, dcur, m, cf, locur, hicur, G[q], Vr[q - VL], pri, dua);
                snew_q = Vr[q - VL];
            } else {
                double vnew;
                if constexpr (K0 && q == 0) xcur = Step::fwd_lds0(dcur, m, c0, locur, hicur, G[q], vcur, vnew, pri, dua);
                else xcur = Step::fwd_lds(xcur, dcur, m, cf, locur, hicur, G[q], vcur, vnew, pri, dua);
                lds_write_async<q * 512>(aV, vnew);
                snew_q = vnew;
            }
            if constexpr (ADAPT) {
                if (adapt) {
                    // state lanes: column x_q (xprev, gprev) and row vnew_{q+1} (snew); input lanes: column / row u_q
                    const double gnew = G[q], out = xcur;
                    const double t = group_matvec<W, 16>(mtr, is_x ? gnew : 0.0, 0.0);  // [A'; B'] g_{q+1}
                    const double dgx = dgr * (is_x ? xprev : out);                       // Q.*x_q | R.*u_q
                    const double aty = is_x ? (t - gprev) : (gnew + t);
                    a_dn = fmax(fmax(a_dn, fabs(dgx)), fabs(aty));
                    a_dr = fmax(a_dr, fabs(2.0 * dgx + aty));
                    a_pr = fmax(a_pr, fabs(is_x ? snew_q : (out - snew_q)));
                    a_pn = fmax(fmax(a_pn, fabs(snew_q)), is_x ? 0.0 : fabs(out));
                    gprev = gnew;
                }
            }
            if constexpr (FAM) {  // xcur: x_{q+1} on state lanes, u_q on input lanes -- this slot's element
                double gcn, gln;
                const double l = families(xcur, GCr[q], GLr[q], gcn, gln, q + 1);
                if (row_ok) {
                    GCr[q] = gcn;
                    GLr[q] = gln;
                    LX[q] = l;
                }
            }
            dcur = dn;
            vcur = vn;
#if TINY_LDS_START
            acur = an;
#endif
            if constexpr (!CT || IKBND) {
                locur = lon;
                hicur = hin;
            }
        };
        constexpr int DF = D_FIRST < NS ? D_FIRST : NS;
        constexpr int NG = 1 + (NS - DF + D_GROUP - 1) / D_GROUP;
        static_for<0, NG>([&](auto Gi) {
            constexpr int s0 = Gi.value == 0 ? 0 : DF + (Gi.value - 1) * D_GROUP;
            constexpr int s1 = Gi.value == 0 ? DF : ((s0 + D_GROUP < NS) ? s0 + D_GROUP : NS);
            if (TINY_RARE(may)) {
                // Stale copy of the group's slots (still holding the previous iterate) before the blocks overwrite them.
                // Rare path: the addresses are rebuilt from an opaque copy of the lane offset so that the compiler does
                // not keep one pointer per slot alive across the iteration loop.
                // (ADAPT: the check after an adaptation scales the dual residual with the NEW rho, which this sweep does not
                // know yet -- no early "cannot converge" verdict in those iterations)
                if constexpr (s0 > 0) {
                    if (!adapt) {
                        const bool bad = !((pri < p.abs_pri_tol) && (dua * rho < p.abs_dua_tol));
#if TINY_REFILL
                        may = __builtin_amdgcn_readfirstlane((int)wave_may_converge_d(__ballot(bad), __ballot(REFILL ? chk : active))) != 0;
#elif TINY_LEAN_PARK
                        may = __builtin_amdgcn_readfirstlane((int)wave_may_converge_d32(__ballot(bad), __ballot(active))) != 0;
#else
                        may = __builtin_amdgcn_readfirstlane((int)((ILIN || ITRAJ || IKBND) ? wave_may_converge_d32(__ballot(bad), __ballot(active)) : wave_may_converge_d(__ballot(bad), __ballot(active)))) != 0;
#endif
                    }
                }
                if (TINY_RARE(may)) {
#if TINY_REFILL
                    unsigned vo = REFILL ? row_offset(cur) + (unsigned)(koff * 64) : voff;
#else
                    unsigned vo = voff;
#endif
                    double *base = gV1u;
                    asm volatile("" : "+v"(vo), "+s"(base));
                    // Only for instances that are still iterating: a zombie's slots hold iterates it computed AFTER it converged,
                    // and its own stale copy -- the previous iterate of the sweep in which it converged, its canonical v|z
                    // (admm.cpp:181-197) -- must survive the later sweeps of its wavefront's other instances.
                    if (active) static_for<s0, s1>([&](auto S) { (base + S.value * 64)[vo] = vget(S); });
                }
            }
            static_for<s0, s1>([&](auto S) { fstep(S); });
        });
#if TINY_REFILL
        if constexpr (REFILL) {
            if (active) it_done += 1;
        } else {
            if (active) it_done = it1;  // admm.cpp:143
        }
#elif TINY_LEAN_HOIST
        if constexpr (!NO_CTL) {
            if (active) it_done = it1;  // (lean rounds: once behind their loop)
        }
#else
        if (active) it_done = it1;  // admm.cpp:143
#endif
#if TINY_LEAN_PARK
        if constexpr (SH_F && !SH_B) unpark();  // (the last round of a run: Vx[] is dead from here on)
#endif

        // ---------------- adaptive rho (admm.cpp:147-174), as in k_admm_solve_adapt
        const double nrho_lin = nrho, rhom_lin = rhom, pnref_lin = pnref;  // what update_linear_cost used this iteration
        if constexpr (ADAPT) {
            if (adapt) {
                const double x_last = xcur, g_last = gprev;  // x_{N-1}, g_{N-1} on state lanes
                // column block x_{N-1}: Pinf x + Q.*x - g_{N-1} with the CURRENT (adapted) Pinf (rho_benchmark.cpp:112)
                double pr[16];
                const double delta = rho - rho0;
                static_for<0, 16>([&](auto K) {
                    constexpr int o = K.value * 16;
                    pr[K.value] = K.value < NXU ? fma(delta, sAd[4 * 256 + o + r], sAd[3 * 256 + o + r]) : 0.0;
                });
                const double pxl = group_matvec<W, 16>(pr, is_x ? x_last : 0.0, 0.0);
                if (is_x) {
                    const double qv = dgr * x_last;
                    a_dn = fmax(fmax(fmax(a_dn, fabs(pxl)), fabs(qv)), fabs(g_last));
                    a_dr = fmax(a_dr, fabs(pxl + qv - g_last));
                }
                const double pri_res = group_max<W>(a_pr), pri_norm = group_max<W>(a_pn);
                const double dual_res = group_max<W>(a_dr), dual_norm = group_max<W>(a_dn);
                const double eps = 1e-10;  // rho_benchmark.cpp:190-197
                const double normalized_pri = pri_res / (pri_norm + eps);
                const double normalized_dual = dual_res / (dual_norm + eps);
                const double ratio = normalized_pri / (normalized_dual + eps);
                double new_rho = rho * sqrt(ratio);
                if (p.rho_clip) new_rho = fmin(fmax(new_rho, p.rho_min), p.rho_max);
                if (active) {  // (rho is unchanged for instances that are no longer iterating)
                    rho = new_rho;
                    nrho = -new_rho;
                    rhom = is_x ? nrho : 0.0;
                    pnref = fma(rho - rho0, dpnref, pnref0);
                }
            }
        }

        // ---------------- R1: termination (admm.cpp:93-101), decided element-wise: one ballot, no reductions
        if (check) {
            const bool below = (pri < p.abs_pri_tol) && (dua * rho < p.abs_dua_tol);
            const bool conv = ((__ballot(below) >> (j * W)) & 0xffffull) == 0xffffull;
#if TINY_REFILL
            if (REFILL ? chk : active) {
#else
            if (active) {
#endif
                snap_pri = pri;
                snap_dua = dua;
                if constexpr (ADAPT) snap_rho = rho;  // cache->rho AFTER the adaptation (admm.cpp:95-96)
                res_valid = true;
                if (conv) {
                    status = 1;  // TINY_SOLVED: this instance stops before the backward pass (admm.cpp:181-192)
                    active = false;
                    pending = true;
                }
            }
        }

        // ---------------- backward sweep (B1, admm.cpp:13-20); linear cost (L1, :77-82) recomputed from V, G
        {
            const unsigned long long wr_d = __ballot(is_u && active);  // a zombie keeps the d of its last real iteration
            // (ITRAJ: the linref of a slot is a read of the wavefront's rows, issued a block ahead of its use like the slack's LDS part --
            // the two the sweep's head needs go out in front of the operator rows; slot S: offset (S + 1) * 512 of aR)
            double lr_head1, lr_head2, lrcur;  // (assigned and read in the ITRAJ form only: no initialiser, so that no other form's code sees them)
            // (... and a step's accumulator start, lr + cb on state lanes and cb on input lanes, is ONE fused multiply-add on a lane constant
            // 1 / 0 -- the same bits as the sum and the select of the shared form: the product is exact, the rows are finite)
            double xsel;
            if constexpr (ITRAJ && !FAM) xsel = is_x ? 1.0 : 0.0;
            if constexpr (ITRAJ) {
                lr_head1 = lds_read_async<NS * 512>(aR);  // (slot S: offset (S + 1) * 512)
                lr_head2 = lds_read_async<(NS - 1) * 512>(aR);
            }
            load_ops(sMb, m);
            auto lr_of = [&](auto S) -> double {  // linref of slot S (its knot differs by lane type) (+ the families' term)
                double base;
                if constexpr (ITRAJ) base = decltype(S)::value == NS - 1 ? lr_head1 : lr_head2;  // (the head's two; the blocks take lrcur)
                else if constexpr (CT) base = lr_c;
                else base = sTl[2 * TOFF + (S.value + 1) * W];
                if constexpr (FAM) base += LX[S.value];
                return base;
            };
            double px, rcur, rnext, acc;
            {   // p_{N-1} (state lanes, admm.cpp:81-82) | r_{N-2} (input lanes) share slot NS-1; then slot NS-2
                // (ADAPT: the linear cost of this iteration was formed BEFORE the adaptation -- rho / pNref of update_linear_cost --,
                // the operators loaded above carry the new Kinf)
                double lrT = is_x ? pnref_lin : lr_of(std::integral_constant<int, NS - 1>{});
                if constexpr (FAM) lrT = is_x ? pnref_lin + LX[NS - 1] : lrT;
                const double lr2 = lr_of(std::integral_constant<int, NS - 2>{});
                double lrmc2;
                if constexpr (ITRAJ && !FAM) lrmc2 = fma(lr2, xsel, cb);  // (with the families: their own select -- LX is theirs)
                else lrmc2 = is_x ? lr2 + cb : cb;
                const double v1 = vget(std::integral_constant<int, NS - 1>{}), v2 = vget(std::integral_constant<int, NS - 2>{});
                double t;
#if TINY_LEAN_SHARE
                // (shared: the start value of block NS-1 goes into the register v_{NS-1} was just read from; the same instructions)
                static_assert(NVR >= 3, "the first three slots of the backward sweep are register slots");
                if constexpr (SH_B && FOLD) {
                    asm("v_add_f64 %[t], %[acc], -%[g1]\n\t"
                        "v_fma_f64 %[px], %[sc], %[t], %[lrT]\n\t"
                        "v_add_f64 %[rn], %[v2], -%[g2]\n\t"
                        "v_fma_f64 %[acc], %[rhom], %[rn], %[lrmc]"
                        : [t] "=&v"(t), [px] "=&v"(px), [acc] "+v"(Vr[NS - 1 - VL]), [rn] "=&v"(rnext)
                        : [g1] "v"(G[NS - 1]), [v2] "v"(v2), [g2] "v"(G[NS - 2]), [sc] "v"(is_x ? nrho : 1.0),
                          [lrT] "v"(is_x ? pnref : 0.0), [rhom] "v"(rhom), [lrmc] "v"(lrmc_f));
                } else if constexpr (SH_B) {
                    asm("v_add_f64 %[t], %[acc], -%[g1]\n\t"
                        "v_fma_f64 %[px], %[nrho], %[t], %[lrT]\n\t"
                        "v_add_f64 %[t], %[v2], -%[g2]\n\t"
                        "v_fma_f64 %[acc], %[rhom], %[t], %[lrmc]\n\t"
                        "v_fma_f64 %[rn], %[nrho], %[t], %[lr]"
                        : [t] "=&v"(t), [px] "=&v"(px), [acc] "+v"(Vr[NS - 1 - VL]), [rn] "=&v"(rnext)
                        : [g1] "v"(G[NS - 1]), [v2] "v"(v2), [g2] "v"(G[NS - 2]), [nrho] "s"(nrho), [lrT] "v"(lrT),
                          [rhom] "v"(rhom), [lrmc] "v"(lrmc2), [lr] "v"(lr2));
                } else
#endif
                if constexpr (ADAPT) {  // (rho is a lane variable here: vector operand)
                    asm("v_add_f64 %[t], %[v1], -%[g1]\n\t"
                        "v_fma_f64 %[px], %[nrho], %[t], %[lrT]\n\t"
                        "v_add_f64 %[t], %[v2], -%[g2]\n\t"
                        "v_fma_f64 %[acc], %[rhom], %[t], %[lrmc]\n\t"
                        "v_fma_f64 %[rn], %[nrho], %[t], %[lr]"
                        : [t] "=&v"(t), [px] "=&v"(px), [acc] "=&v"(acc), [rn] "=&v"(rnext)
                        : [v1] "v"(v1), [g1] "v"(G[NS - 1]), [v2] "v"(v2), [g2] "v"(G[NS - 2]), [nrho] "v"(nrho_lin), [lrT] "v"(lrT),
                          [rhom] "v"(rhom_lin), [lrmc] "v"(lrmc2), [lr] "v"(lr2));
                } else if constexpr (FOLD) {  // (input lanes: px = 1 * t + 0 = t exactly, the r_{N-2} of the folded operator; rn = t)
                    asm("v_add_f64 %[t], %[v1], -%[g1]\n\t"
                        "v_fma_f64 %[px], %[sc], %[t], %[lrT]\n\t"
                        "v_add_f64 %[rn], %[v2], -%[g2]\n\t"
                        "v_fma_f64 %[acc], %[rhom], %[rn], %[lrmc]"
                        : [t] "=&v"(t), [px] "=&v"(px), [acc] "=&v"(acc), [rn] "=&v"(rnext)
                        : [v1] "v"(v1), [g1] "v"(G[NS - 1]), [v2] "v"(v2), [g2] "v"(G[NS - 2]), [sc] "v"(is_x ? nrho : 1.0),
                          [lrT] "v"(is_x ? pnref : 0.0), [rhom] "v"(rhom), [lrmc] "v"(lrmc_f));
                } else {
                    asm("v_add_f64 %[t], %[v1], -%[g1]\n\t"
                        "v_fma_f64 %[px], %[nrho], %[t], %[lrT]\n\t"
                        "v_add_f64 %[t], %[v2], -%[g2]\n\t"
                        "v_fma_f64 %[acc], %[rhom], %[t], %[lrmc]\n\t"
                        "v_fma_f64 %[rn], %[nrho], %[t], %[lr]"
                        : [t] "=&v"(t), [px] "=&v"(px), [acc] "=&v"(acc), [rn] "=&v"(rnext)
                        : [v1] "v"(v1), [g1] "v"(G[NS - 1]), [v2] "v"(v2), [g2] "v"(G[NS - 2]), [nrho] "s"(nrho), [lrT] "v"(lrT),
                          [rhom] "v"(rhom), [lrmc] "v"(lrmc2), [lr] "v"(lr2));
                }
                rcur = px;
            }
            // slack operand of a block's tail: a register, or an LDS read issued one block ahead
            auto vreq = [&](auto S) -> double {
#if TINY_LEAN_PARK
                if constexpr (SH_B && decltype(S)::value >= VLR && decltype(S)::value < VL) return Vx[decltype(S)::value - VLR];
                else
#endif
                if constexpr (decltype(S)::value >= VL) return Vr[decltype(S)::value - VL];
                else return lds_read_async<decltype(S)::value * 512>(aV);
            };
            double v2cur = vreq(std::integral_constant<int, (NS >= 3 ? NS - 3 : 0)>{});
            if constexpr (ITRAJ) lrcur = lds_read_async<(NS - 2) * 512>(aR);  // (slot NS - 3: the first block's)
            lds_wait_ops(m);
#if TINY_LEAN_HOIST
            // Knot 0's dual update, G0 = s - snew (V0 is snew by now), placed here by hand: the first backward block follows the asm
            // statement above directly, and between two asm statements with nothing but the wait in between the compiler puts a hazard
            // s_nop, which this instruction makes unnecessary (in the lean kernels of tinympc_lean_d.hip the scheduler happens to leave
            // it here; with the control hoisted it moved to the loop's end). The same instruction on the same operands.
            if constexpr (LEANI) {
                asm volatile("" : "+v"(G0));
                G0 = G0 - V0;
                asm volatile("" ::"v"(G0));
            }
#endif
            static_for<0, NS - 1>([&](auto I) {
                constexpr int s = NS - 1 - I.value;           // NS-1 .. 1
                constexpr int s2 = s >= 2 ? s - 2 : 0;        // slot feeding the tail (s = 1: any finite t will do)
                constexpr int s3 = s >= 3 ? s - 3 : 0;        // ... of the next block
                // (an asynchronous read MUST be consumed after its wait: the destination of a dead one would be handed to
                // the block's outputs while the read is still in flight)
                double v2n = 0.0;
                if constexpr (s >= 2) v2n = vreq(std::integral_constant<int, s3>{});
                double lrn;  // (ITRAJ: the next block's linref, slot s3; block 1's tail feeds nothing -- it keeps slot 0's)
                // (... with the families block 1 keeps the very value block 2 used, slot 0's read of block 3: the sums with LX[0] and cb are
                // then formed once for both, as the goal form forms them on its lane constant)
                constexpr int LR_LAST = FAM ? 3 : 2;  // the last block that reads ahead
                if constexpr (ITRAJ) {  // (nested: a condition that depends on the step would capture these in every form's lambda)
                    if constexpr (s >= LR_LAST) lrn = lds_read_async<(s3 + 1) * 512>(aR);
                }
                double lr2;
                if constexpr (ITRAJ && FAM) lr2 = lrcur + LX[s2];  // (the slot's row + the families' term: lr_of's sum on the read of a block ago)
                else if constexpr (ITRAJ) lr2 = lrcur;
                else lr2 = lr_of(std::integral_constant<int, s2>{});
                double lrmc2;
                if constexpr (ITRAJ && !FAM) lrmc2 = fma(lr2, xsel, cb);  // (with the families: their own select -- LX is theirs)
                else lrmc2 = is_x ? lr2 + cb : cb;
#if TINY_LEAN_PARK
                if constexpr (SH_B && s >= VLR) {
                    // The shared block below with the run's split: the register of slot s is Vr[s-VL], or Vx[s-VLR] for a converted slot;
                    // the boundary block is VLR (it writes `an` into the scratch accumulator and the LDS slots go on as before).
                    constexpr bool AN_REG = s - 1 >= VLR;
                    constexpr int sn = AN_REG ? s - 1 : s;
                    double &a_s = s >= VL ? Vr[s >= VL ? s - VL : 0] : Vx[s >= VL ? 0 : s - VLR];
                    double &an_s = sn >= VL ? Vr[sn >= VL ? sn - VL : 0] : Vx[sn >= VL ? 0 : sn - VLR];
                    double an_l, rn;
                    static_assert(FOLD, "constant tables only");
                    if constexpr (AN_REG) Step::bwd_fold(a_s, px, rcur, m, v2cur, G[s2], rhom, lrmc_f, an_s, rn);
                    else Step::bwd_fold(a_s, px, rcur, m, v2cur, G[s2], rhom, lrmc_f, an_l, rn);
                    if constexpr (!AN_REG) acc = an_l;
                    px = a_s;
                    rcur = rnext;
                    rnext = rn;
                    v2cur = v2n;
                    return;
                }
#elif TINY_LEAN_SHARE
                if constexpr (SH_B && s >= VL) {
                    // The shared block of a register slot: Vr[s-VL] holds the start value (its v_s was consumed two blocks ago) and
                    // becomes [p_s | d_s]; the tail's start value for block s-1 goes into that slot's register where it has one. No d
                    // store. (The blocks down to VL+3 issue no LDS instruction and keep their wait all the same: see the top of the file.)
                    constexpr bool AN_REG = s - 1 >= VL;
                    double &an_s = Vr[AN_REG ? s - 1 - VL : 0];
                    double an_l, rn;
                    // (s = 1 with a register slot 0: v2cur is v_0, whose register is this block's `an`; any finite t will do)
                    const double v2op = (s == 1 && AN_REG) ? rhom : v2cur;
                    if constexpr (FOLD && AN_REG) Step::bwd_fold(Vr[s - VL], px, rcur, m, v2op, G[s2], rhom, lrmc_f, an_s, rn);
                    else if constexpr (FOLD) Step::bwd_fold(Vr[s - VL], px, rcur, m, v2op, G[s2], rhom, lrmc_f, an_l, rn);
                    else if constexpr (AN_REG) Step::bwd(Vr[s - VL], px, rcur, m, v2op, G[s2], rhom, lrmc2, nrho, lr2, an_s, rn);
                    else Step::bwd(Vr[s - VL], px, rcur, m, v2op, G[s2], rhom, lrmc2, nrho, lr2, an_l, rn);
                    if constexpr (!AN_REG) acc = an_l;
                    px = Vr[s - VL];
                    rcur = rnext;
                    rnext = rn;
                    v2cur = v2n;
                    return;
                }
#endif
                double a = acc, an, rn;
                if constexpr (ADAPT) Step::bwd_v(a, px, rcur, m, v2cur, G[s2], rhom_lin, lrmc2, nrho_lin, lr2, an, rn);
                else if constexpr (FOLD) Step::bwd_fold(a, px, rcur, m, v2cur, G[s2], rhom, lrmc_f, an, rn);
                else Step::bwd(a, px, rcur, m, v2cur, G[s2], rhom, lrmc2, nrho, lr2, an, rn);
#if TINY_TRIM_DSTORE
                if constexpr (NO_CTL) lds_write_async<s * DS * 8>(aDw, a);  // d_s, or a dump row (see `dstore` at the top of the file)
                else lds_write_masked<s * DS * 8>(aD, a, wr_d);
#else
                lds_write_masked<s * DS * 8>(aD, a, wr_d);  // d_s
#endif
                px = a;
                rcur = rnext;
                rnext = rn;
                acc = an;
                v2cur = v2n;
                if constexpr (ITRAJ) {
                    if constexpr (s >= LR_LAST) lrcur = lrn;
                }
            });
#if TINY_LEAN_SHARE
            if constexpr (SH_B && VL == 0) Step::bwd_last(Vr[0], px, rcur, m);  // (slot 0 is a register slot: d_0 stays in it)
            else
#endif
            {
                double a = acc;
                Step::bwd_last(a, px, rcur, m);
#if TINY_TRIM_DSTORE
                if constexpr (NO_CTL) lds_write_async<0>(aDw, a);
                else lds_write_masked<0>(aD, a, wr_d);
#else
                lds_write_masked<0>(aD, a, wr_d);  // d_0
#endif
            }
        }
#if TINY_LEAN
        return false;
    };
    // admm.cpp:129. `nres`: the next iteration, counted from 1, whose residuals something reads (need_res, see the top of the file);
    // the rounds before it are lean, and so is everything behind the last one. All of it scalar.
    const bool reachable = p.abs_pri_tol > 0.0 && p.abs_dua_tol > 0.0;
    const int last_check = ct > 0 ? (max_iter / ct) * ct : 0;
    for (int it = 0; max_iter > 0;) {
        int nres = max_iter + 1;
        if (ct > 0 && reachable) nres = (it / ct + 1) * ct;
        else if (last_check > it) nres = last_check;
        const int lean_end = __builtin_amdgcn_readfirstlane(nres - 1 < max_iter ? nres - 1 : max_iter);
#if TINY_LEAN_HOIST
        if (it < lean_end) {
            // what can end a run of lean rounds, or ask it for a write-back, is decided before the run starts: once, here
            if (iteration(std::integral_constant<int, 2>{}, it)) break;
#if TINY_TRIM_DSTORE
            {   // `active` is fixed for the run, and some instance of the wavefront is live (the control above would have ended the solve)
                const unsigned long long live = __ballot(active);
                const unsigned lm = (unsigned)(live & 1ull) | (unsigned)((live >> 15) & 2ull) | (unsigned)((live >> 30) & 4ull) | (unsigned)((live >> 45) & 8ull);
                const int first = __builtin_ctz(lm | 16u);
                // dump lanes: the columns of this lane's own instance (row -1), of the instance two further (row -1) and of that one again
                // (row -2): with four live instances the 24 dump lanes and the 8 storing lanes of a half-wavefront hit 32 different
                // addresses in 64 different banks. An instance that is not live is replaced by the first live one.
                const int cls = (r / NU) % 3;
                int jt = cls == 0 ? j : (j ^ 2);
                if (((lm >> jt) & 1u) == 0u) jt = first & 3;
                const unsigned dump = lds_addr(sD) + (unsigned)((jt * NU + r % NU) * 8) - (unsigned)((cls == 2 ? 2 : 1) * DS * 8);
                aDw = (is_u && active) ? aD : dump;
            }
#endif
#if TINY_LEAN_SHARE
            // Entry of a run: d_s of the register slots from LDS into the slots' registers (the old slack is dead, see the top of the
            // file), once per run; then the shared rounds and, last, the round whose backward sweep puts everything back in place.
            static_for<0, NVR>([&](auto S) { Vr[S.value] = lds_read_async<(VL + S.value) * DS * 8>(aD); });
#if TINY_LEAN_PARK
            // (... and of the slots that are register slots inside the run only; their old slack in LDS is dead in the same way)
            static_for<0, NVX>([&](auto S) { Vx[S.value] = lds_read_async<(VLR + S.value) * DS * 8>(aD); });
            lds_wait();
            static_for<0, NVX>([&](auto S) {
                double &vx = Vx[decltype(S)::value];
                asm volatile("" : "+v"(vx));
            });
            park();
#else
            lds_wait();
#endif
            static_for<0, NVR>([&](auto S) {  // (the reads are consumed behind their wait)
                double &vr = Vr[decltype(S)::value];
                asm volatile("" : "+v"(vr));
            });
            for (; it < lean_end - 1; ++it) (void)iteration(std::integral_constant<int, 3>{}, it);
            (void)iteration(std::integral_constant<int, 4>{}, it);
            ++it;
#else
            for (; it < lean_end; ++it) (void)iteration(std::true_type{}, it);
#endif
            if (active) it_done = __builtin_amdgcn_readfirstlane(it);  // admm.cpp:143, for the whole run
        }
        if (iteration(std::false_type{}, it)) break;
#else
        bool over = false;
        for (; it < lean_end; ++it) {
            if (iteration(std::true_type{}, it)) {
                over = true;
                break;
            }
        }
        if (over || iteration(std::false_type{}, it)) break;
#endif
        ++it;
    }
#else
    }
#endif
    lds_wait();
#ifdef TINY_CLOCK_STAMP
    // Delta s_memtime (shader cycles) and Delta s_memrealtime (a constant 100 MHz) around the iteration loop, one pair per
    // wavefront, into a buffer of their own that nothing else reads (SolveParams::scratch, unused by this layout otherwise)
    const unsigned long long ck_t1 = __builtin_amdgcn_s_memtime(), ck_r1 = __builtin_amdgcn_s_memrealtime();
#endif

    // A converged solve returned before v <- vnew (admm.cpp:181-197): its canonical v|z is the previous iterate, i.e. the
    // stale copy. (The write-back above stored vnew there; this wave wrote both, in program order.)
#if TINY_REFILL
    if constexpr (REFILL) return;  // (every row was finished inside the loop)
#endif
    if (inst_ok && status == 1 && r < NXU) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        const int rows = is_x ? N : NS;
        double *const wV = p.V + ((size_t)grp * v_rows(N) + V_PAD) * 64 + lane;
        const double *const wV2 = p.V2 + ((size_t)grp * v_rows(N) + V_PAD) * 64 + lane;
        for (int kn = 0; kn < rows; ++kn) wV[kn * 64] = wV2[kn * 64];
    }

    const double res_px = group_max<W>(is_x ? snap_pri : 0.0), res_pu = group_max<W>(is_u ? snap_pri : 0.0);
    const double rho_res = ADAPT ? snap_rho : rho;
    const double res_dx = group_max<W>(is_x ? snap_dua : 0.0) * rho_res, res_du = group_max<W>(is_u ? snap_dua : 0.0) * rho_res;

#ifdef TINY_CLOCK_STAMP
    // One record per wavefront, into a buffer of its own that nothing else reads (SolveParams::scratch, unused by this layout
    // otherwise): shader cycles and 100 MHz ticks of the iteration loop (the final round's write-back included), and the ticks of
    // the phases around it -- entry -> the prologue's barrier (operators, d and the LDS part of the slack in), barrier -> loop
    // (the register part of the state in), loop end -> here (residual reductions), absolute entry / exit times.
    if (p.scratch && lane == 0) {
        unsigned long long *ck = reinterpret_cast<unsigned long long *>(p.scratch) + 8 * (size_t)grp;
        ck[0] = ck_t1 - ck_t0;
        ck[1] = ck_r1 - ck_r0;
        ck[2] = ck_barrier - ck_entry;
        ck[3] = ck_r0 - ck_barrier;
        ck[4] = __builtin_amdgcn_s_memrealtime() - ck_r1;
        ck[5] = ck_entry;
        ck[6] = __builtin_amdgcn_s_memrealtime();
        ck[7] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) | ((unsigned long long)__builtin_amdgcn_s_getreg((3 << 11) | 20) << 32);  // HW_ID, XCC_ID
    }
#endif
#if TINY_LEAN_PARK
    // (the instance's number again, from an opaque copy of the lane: the 64-bit index does not live across the iteration loop)
    int lane_e = lane;
    asm volatile("" : "+v"(lane_e));
    const long inst_e = grp * IPW + (lane_e >> 4);
    if (inst_ok && r == 0) {
        p.istats[inst_e * 2 + 0] = it_done;
        p.istats[inst_e * 2 + 1] = status;
        if (res_valid) {
            p.dstats[inst_e * 4 + 0] = res_px;
            p.dstats[inst_e * 4 + 1] = res_dx;
            p.dstats[inst_e * 4 + 2] = res_pu;
            p.dstats[inst_e * 4 + 3] = res_du;
        }
    }
#else
    if (inst_ok && r == 0) {
        if constexpr (ADAPT) p.rho_inst[inst] = rho;
        p.istats[inst * 2 + 0] = it_done;
        p.istats[inst * 2 + 1] = status;
        if (res_valid) {
            p.dstats[inst * 4 + 0] = res_px;
            p.dstats[inst * 4 + 1] = res_dx;
            p.dstats[inst * 4 + 2] = res_pu;
            p.dstats[inst * 4 + 3] = res_du;
        }
    }
#endif
}

#if TINY_LEAN
// (the lean translation unit, tinympc_lean_d.hip: the plain kernel and its per-instance goal form with lean sweeps; tinympc_plan.hip
// decides when -- lean_applies; tinympc_lstart_d.hip: the same under the names of its variant)
#if TINY_LEAN_PARK
#define k_admm_solve_d_lean k_admm_solve_d_lean_park
#define k_admm_solve_d_gbnd_lean k_admm_solve_d_gbnd_lean_park
#define launch_solve_d_lean launch_solve_d_lean_park
// (the LDS plan is the shared kernels': no row moves, the run's split only changes which instructions touch them)
static_assert(d_vl(4, 50, true, 4) == 25, "quadrotor N=50: 25 slack slots in LDS with four wavefronts per workgroup");
#elif TINY_LEAN_SHARE
#define k_admm_solve_d_lean k_admm_solve_d_lean_share
#define k_admm_solve_d_gbnd_lean k_admm_solve_d_gbnd_lean_share
#define launch_solve_d_lean launch_solve_d_lean_share
// (the LDS plan is the trimmed kernels': the slack slots and every row of d keep their places, fewer instructions touch them)
static_assert(d_vl(4, 50, true, 4) == 25, "quadrotor N=50: 25 slack slots in LDS with four wavefronts per workgroup");
#elif TINY_LEAN_TRIM
#define k_admm_solve_d_lean k_admm_solve_d_lean_trim
#define k_admm_solve_d_gbnd_lean k_admm_solve_d_gbnd_lean_trim
#define launch_solve_d_lean launch_solve_d_lean_trim
// (... and the two dump rows in front of d, 32 doubles, come out of the 44 the plan had left)
static_assert(d_vl(4, 50, true, 4) == 25, "quadrotor N=50: 25 slack slots in LDS with four wavefronts per workgroup");
#elif TINY_LEAN_START
#define k_admm_solve_d_lean k_admm_solve_d_lean_start
#define k_admm_solve_d_gbnd_lean k_admm_solve_d_gbnd_lean_start
#define launch_solve_d_lean launch_solve_d_lean_start
// (the quadrotor's plan has 1,644 doubles per wavefront behind d with the 16 of the table taken out: 25 slots of 64 still fit)
static_assert(d_vl(4, 50, true, 4) == 25, "quadrotor N=50: 25 slack slots in LDS with four wavefronts per workgroup");
#endif
template <int NX, int NU, int N, bool CT, int WPG, int VL>
__global__ void __launch_bounds__(64 * WPG) __attribute__((amdgpu_waves_per_eu(2, 2))) k_admm_solve_d_lean(const SolveParams p) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    k_admm_solve_d_body<NX, NU, N, CT, WPG, VL>(p, smem);
}
template <int NX, int NU, int N, int WPG, int VL>
__global__ void __launch_bounds__(64 * WPG) __attribute__((amdgpu_waves_per_eu(2, 2))) k_admm_solve_d_gbnd_lean(const SolveParams p) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    k_admm_solve_d_body<NX, NU, N, true, WPG, VL, false, false, true, false, false, true>(p, smem);
}

__host__ __device__ constexpr int d_wpg(int nu, int N, bool ct) { return d_vl(nu, N, ct, 4) >= 0 ? 4 : 8; }  // (as in the plain translation unit)

template <int NX, int NU, int N, bool CT>
static hipError_t launch_d_one(const SolveParams &p, hipStream_t stream) {
    constexpr int WPG = d_wpg(NU, N, CT);
    constexpr int VL = d_vl(NU, N, CT, WPG);
    if constexpr (VL < 0) {
        return hipErrorInvalidValue;
    } else {
        constexpr size_t lds = d_lds_bytes(NU, N, CT, WPG, VL);
        static size_t lds_set_l[16] = {0}, lds_set_lgoal[16] = {0};
        const int wgs = (p.groups + WPG - 1) / WPG;
        if (p.x0_mirror || p.u0_host || p.refill_next) return hipErrorInvalidValue;  // (the plan keeps those on their own kernels)
        if (p.iref_pn) {  // per-instance goals (constant tables only)
            if constexpr (!CT) {
                return hipErrorInvalidValue;
            } else {
                if (!p.iref_lr || !p.ibnd) return hipErrorInvalidValue;
                auto fn = &k_admm_solve_d_gbnd_lean<NX, NU, N, WPG, VL>;
                hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void *>(fn), lds, lds_set_lgoal);
                if (e != hipSuccess) return e;
                hipLaunchKernelGGL(fn, dim3(wgs), dim3(64 * WPG), lds, stream, p);
            }
        } else {
            auto fn = &k_admm_solve_d_lean<NX, NU, N, CT, WPG, VL>;
            hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void *>(fn), lds, lds_set_l);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(fn, dim3(wgs), dim3(64 * WPG), lds, stream, p);
        }
        return hipGetLastError();
    }
}

#if TINY_LEAN_PARK
hipError_t launch_solve_d_lean(const SolveParams &p, hipStream_t stream) {  // (the one shape with LDS slots, constant tables: see the plan)
    if (p.nx == 12 && p.nu == 4 && p.N == 50 && p.const_tables) return launch_d_one<12, 4, 50, true>(p, stream);
    return hipErrorInvalidValue;
}
#else
hipError_t launch_solve_d_lean(const SolveParams &p, hipStream_t stream) {  // (the shapes of TINY_D_SHAPES in the plain translation unit)
    if (p.nx == 12 && p.nu == 4 && p.N == 50) return p.const_tables ? launch_d_one<12, 4, 50, true>(p, stream) : launch_d_one<12, 4, 50, false>(p, stream);
    if (p.nx == 4 && p.nu == 1 && p.N == 20) return p.const_tables ? launch_d_one<4, 1, 20, true>(p, stream) : launch_d_one<4, 1, 20, false>(p, stream);
    if (p.nx == 4 && p.nu == 1 && p.N == 10) return p.const_tables ? launch_d_one<4, 1, 10, true>(p, stream) : launch_d_one<4, 1, 10, false>(p, stream);
    return hipErrorInvalidValue;
}
#endif
#else  // the plain and the slot-refill kernels, their launchers, the run-time specialised entry point
#ifndef TINY_JIT
#if TINY_REFILL
template <int NX, int NU, int N, bool CT, int WPG, int VL>
__global__ void __launch_bounds__(64 * WPG) __attribute__((amdgpu_waves_per_eu(2, 2))) k_admm_solve_d_refill(const SolveParams p) {
#else
template <int NX, int NU, int N, bool CT, int WPG, int VL, bool HOSTX = false>
__global__ void __launch_bounds__(64 * WPG) __attribute__((amdgpu_waves_per_eu(2, 2))) k_admm_solve_d(const SolveParams p) {
#endif
    extern __shared__ __attribute__((aligned(16))) double smem[];
#if TINY_REFILL
    k_admm_solve_d_body<NX, NU, N, CT, WPG, VL, false, false, true, false, true>(p, smem);
#else
    k_admm_solve_d_body<NX, NU, N, CT, WPG, VL, false, false, true, HOSTX>(p, smem);
#endif
}
#if TINY_REFILL
// Slot refill for the per-instance goal form (k_admm_solve_d_gbnd's launches): a row that takes the next instance of the batch takes
// that instance's lr_c / pNref / lo_c / hi_c and folded accumulator start with it.
template <int NX, int NU, int N, int WPG, int VL>
__global__ void __launch_bounds__(64 * WPG) __attribute__((amdgpu_waves_per_eu(2, 2))) k_admm_solve_d_refill_gbnd(const SolveParams p) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    k_admm_solve_d_body<NX, NU, N, true, WPG, VL, false, false, true, false, true, true>(p, smem);
}
#endif
#if !TINY_REFILL
// The per-instance goal form (one goal per instance from tinympc_set_x_ref_batch and / or one box per instance from
// tinympc_set_bound_constraints_batch; shared references and bounds that are constant over the horizon fill the rest): the plain
// constant-table kernel with the instance's lr_c / pNref / lo_c / hi_c loaded per lane at kernel start.
template <int NX, int NU, int N, int WPG, int VL>
__global__ void __launch_bounds__(64 * WPG) __attribute__((amdgpu_waves_per_eu(2, 2))) k_admm_solve_d_gbnd(const SolveParams p) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    k_admm_solve_d_body<NX, NU, N, true, WPG, VL, false, false, true, false, false, true>(p, smem);
}
#endif
#endif

#ifdef TINY_JIT
}  // namespace tinympc
// The one kernel of a run-time specialised module: a fixed C name, static LDS (its size is known here).
#ifndef TINY_JIT_WPS
#define TINY_JIT_WPS 2  // wavefronts per SIMD: 2 (256 registers each), or 1 (512) for horizons whose duals need them
#endif
#ifndef TINY_JIT_WPG
#define TINY_JIT_WPG (4 * TINY_JIT_WPS)
#endif
// the entry point: `tinympc_jit_solve` as a run-time specialisation (tinympc_jit.hip looks it up by that name), the name the build
// gives it as a compiled-in one
#ifdef TINY_BUILTIN
#define TINY_KERNEL_NAME TINY_BUILTIN_NAME
#else
#define TINY_KERNEL_NAME tinympc_jit_solve
#endif
#ifndef TINY_JIT_IMOD
#define TINY_JIT_IMOD 0
#endif
#if TINY_JIT_IMOD && TINY_REFILL
#error "per-instance models: no slot-refill variant"
#endif
#ifndef TINY_JIT_ILIN
#define TINY_JIT_ILIN 0
#endif
#if TINY_JIT_ILIN && TINY_REFILL
#error "per-instance linear rows: no slot-refill variant"
#endif
#if TINY_REFILL && ((defined(TINY_JIT_IKBND) && TINY_JIT_IKBND) || (defined(TINY_JIT_ITRAJ) && TINY_JIT_ITRAJ)) && !(defined(TINY_JIT_IGOAL) && TINY_JIT_IGOAL)
#error "slot refill for per-instance trajectories / bounds per knot: forms of the goal form (-DTINY_JIT_IGOAL=1)"
#endif
extern "C" __global__ void __launch_bounds__(64 * TINY_JIT_WPG) __attribute__((amdgpu_waves_per_eu(TINY_JIT_WPS, TINY_JIT_WPS)))
TINY_KERNEL_NAME(const tinympc::SolveParams p) {
#ifndef TINY_JIT_CT
#define TINY_JIT_CT 1
#endif
    constexpr bool CTJ = TINY_JIT_CT != 0;  // bounds / references constant over the horizon
    constexpr int WPGJ = TINY_JIT_WPG;  // wavefronts per workgroup (4, or 8 where only that LDS plan fits)
#ifndef TINY_JIT_FAM
#define TINY_JIT_FAM 0
#endif
    constexpr bool FAMJ = TINY_JIT_FAM != 0;  // cone / linear-inequality families
#ifndef TINY_JIT_ADAPT
#define TINY_JIT_ADAPT 0
#endif
    constexpr bool ADJ = TINY_JIT_ADAPT != 0;  // adaptive rho
    constexpr bool IMJ = TINY_JIT_IMOD != 0;  // per-instance models (implies the goal form)
#ifndef TINY_JIT_ICONE
#define TINY_JIT_ICONE 0
#endif
#ifndef TINY_JIT_IKNOT
#define TINY_JIT_IKNOT 0
#endif
    constexpr int ILJ = TINY_JIT_ILIN;  // per-instance linear rows: the mode's row count (with -DTINY_JIT_FAM=1 -DTINY_JIT_IGOAL=1); 0: off
    constexpr int KNJ = TINY_JIT_IKNOT != 0 ? TINY_JIT_N : 0;  // ... in the per-knot form (-DTINY_JIT_IKNOT=1): the slots a wavefront stages
#ifndef TINY_JIT_ITRAJ
#define TINY_JIT_ITRAJ 0
#endif
    constexpr bool ITJ = TINY_JIT_ITRAJ != 0;  // per-instance trajectories (with -DTINY_JIT_IGOAL=1): the wavefront's own linref rows
#ifndef TINY_JIT_IKBND
#define TINY_JIT_IKBND 0
#endif
    constexpr bool IBJ = TINY_JIT_IKBND != 0;  // per-knot bounds per instance (with -DTINY_JIT_IGOAL=1): the wavefront's own clamp rows
    constexpr int VLJ = tinympc::d_vl(TINY_JIT_NU, TINY_JIT_N, CTJ, WPGJ, 4 * TINY_JIT_WPS, FAMJ, ADJ, IMJ, ILJ, KNJ, ITJ, IBJ);
    static_assert(VLJ >= 0, "shape does not fit the layout-D plan");
    __shared__ __attribute__((aligned(16))) double smem_jit[tinympc::d_lds_bytes(TINY_JIT_NU, TINY_JIT_N, CTJ, WPGJ, VLJ, FAMJ, ADJ, IMJ, ILJ, KNJ, ITJ, IBJ) / sizeof(double)];
#if TINY_REFILL
#ifndef TINY_JIT_REFILL
#define TINY_JIT_REFILL 0
#endif
#if defined(TINY_JIT_IGOAL) && TINY_JIT_IGOAL
#if !TINY_JIT_REFILL || !TINY_JIT_CT || TINY_JIT_FAM || TINY_JIT_ADAPT
#error "slot refill for the goal form: the box path with constant tables"
#endif
    // (the goal form: a row's four lane constants and its folded accumulator start follow the instance it takes; its trajectory and
    // per-knot bounds forms: the lane constants they have, and the row's column of the wavefront's linref / clamp rows)
    tinympc::k_admm_solve_d_body<TINY_JIT_NX, TINY_JIT_NU, TINY_JIT_N, true, WPGJ, VLJ, false, false, TINY_JIT_WPS == 2, false, true, true, false, 0, false, false, ITJ, IBJ>(p, smem_jit);
#else
    tinympc::k_admm_solve_d_body<TINY_JIT_NX, TINY_JIT_NU, TINY_JIT_N, CTJ, WPGJ, VLJ, FAMJ, ADJ, TINY_JIT_WPS == 2, false, TINY_JIT_REFILL != 0>(p, smem_jit);
#endif
#else
#ifndef TINY_JIT_IGOAL
#define TINY_JIT_IGOAL 0
#endif
    tinympc::k_admm_solve_d_body<TINY_JIT_NX, TINY_JIT_NU, TINY_JIT_N, CTJ, WPGJ, VLJ, FAMJ, ADJ, TINY_JIT_WPS == 2, false, false,
                                 TINY_JIT_IGOAL != 0 || IMJ, IMJ, ILJ, TINY_JIT_ICONE != 0, TINY_JIT_IKNOT != 0, ITJ, IBJ>(p, smem_jit);
#endif
}
namespace tinympc {
#else
// ------------------------------------------------------------------------------------------------------------
// Host side: the instantiation table. A shape runs on layout D only if it was compiled in.
// ------------------------------------------------------------------------------------------------------------
// Wavefronts per workgroup: four where the LDS plan allows it, else eight. Small workgroups spread a batch over the CUs
// wavefront by wavefront: 4,096 quadrotor instances are 1,024 wavefronts = 256 workgroups of four = ONE wavefront per SIMD on
// every CU (6.4 us per iteration, 634 M iterations/s), where 128 workgroups of eight filled half the chip with two wavefronts
// per SIMD (10.1 us, 406 M); full batches gain a few percent from the finer tail (profiles/r02_layout_sweep.txt).
__host__ __device__ constexpr int d_wpg(int nu, int N, bool ct) { return d_vl(nu, N, ct, 4) >= 0 ? 4 : 8; }

#if !TINY_REFILL
// Slot refill launches one resident set: 2 wavefronts per SIMD x 4 SIMDs x the device's CUs, in workgroups of wpg.
int solve_d_resident_workgroups(int wpg) {
    // compute units of the CURRENT device, cached per device id (devices of one node may differ in partition mode); the slots
    // are written at most once each with the same value, so a relaxed atomic is all the synchronisation they need
    static std::atomic<int> cus_of[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    int cus = cus_of[dev].load(std::memory_order_relaxed);
    if (cus == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cus_of[dev].store(cus = n, std::memory_order_relaxed);
    }
    return cus * 8 / wpg;
}
int solve_d_wavefronts_per_workgroup(int nu, int N, bool const_tables) { return d_wpg(nu, N, const_tables); }

#endif
#if TINY_REFILL
// (the slot-refill translation unit, tinympc_solve_dr.hip: one resident set of wavefronts, tinympc_plan.hip decides when)
template <int NX, int NU, int N, bool CT>
static hipError_t launch_d_one(const SolveParams &p, hipStream_t stream) {
    constexpr int WPG = d_wpg(NU, N, CT);
    constexpr int VL = d_vl(NU, N, CT, WPG);
    if constexpr (VL < 0) {
        return hipErrorInvalidValue;
    } else {
        constexpr size_t lds = d_lds_bytes(NU, N, CT, WPG, VL);
        static size_t lds_set_r[16] = {0}, lds_set_rgoal[16] = {0};
        const int wgs = (p.groups + WPG - 1) / WPG;
        const int resident = solve_d_resident_workgroups(WPG);
        if (p.iref_pn) {  // per-instance goals (constant tables only; the guards of the plain goal launch)
            if constexpr (!CT) {
                return hipErrorInvalidValue;
            } else {
                if (p.x0_mirror || p.u0_host || !p.iref_lr || !p.ibnd) return hipErrorInvalidValue;
                auto fn = &k_admm_solve_d_refill_gbnd<NX, NU, N, WPG, VL>;
                hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void *>(fn), lds, lds_set_rgoal);
                if (e != hipSuccess) return e;
                hipLaunchKernelGGL(fn, dim3(wgs < resident ? wgs : resident), dim3(64 * WPG), lds, stream, p);
            }
            return hipGetLastError();
        }
        auto fn = &k_admm_solve_d_refill<NX, NU, N, CT, WPG, VL>;
        hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void *>(fn), lds, lds_set_r);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(fn, dim3(wgs < resident ? wgs : resident), dim3(64 * WPG), lds, stream, p);
        return hipGetLastError();
    }
}
#else
template <int NX, int NU, int N, bool CT>
static hipError_t launch_d_one(const SolveParams &p, hipStream_t stream) {
    constexpr int WPG = d_wpg(NU, N, CT);
    constexpr int VL = d_vl(NU, N, CT, WPG);
    if constexpr (VL < 0) {
        return hipErrorInvalidValue;
    } else {
        constexpr size_t lds = d_lds_bytes(NU, N, CT, WPG, VL);
        static size_t lds_set[16] = {0}, lds_set_x[16] = {0}, lds_set_goal[16] = {0};
        const int wgs = (p.groups + WPG - 1) / WPG;
        if (p.iref_pn) {  // per-instance goals (constant tables only; the plan never combines them with the zero-copy tick)
            if constexpr (!CT) {
                return hipErrorInvalidValue;
            } else {
                if (p.x0_mirror || p.u0_host || !p.iref_lr || !p.ibnd) return hipErrorInvalidValue;
                auto fn = &k_admm_solve_d_gbnd<NX, NU, N, WPG, VL>;
                hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void *>(fn), lds, lds_set_goal);
                if (e != hipSuccess) return e;
                hipLaunchKernelGGL(fn, dim3(wgs), dim3(64 * WPG), lds, stream, p);
            }
        } else if (p.x0_mirror || p.u0_host) {  // (the batched zero-copy tick)
            auto fn = &k_admm_solve_d<NX, NU, N, CT, WPG, VL, true>;
            hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void *>(fn), lds, lds_set_x);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(fn, dim3(wgs), dim3(64 * WPG), lds, stream, p);
        } else {
            auto fn = &k_admm_solve_d<NX, NU, N, CT, WPG, VL>;
            hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void *>(fn), lds, lds_set);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(fn, dim3(wgs), dim3(64 * WPG), lds, stream, p);
        }
        return hipGetLastError();
    }
}

#endif

#define TINY_D_SHAPES(X) \
    X(12, 4, 50)         \
    X(4, 1, 20)          \
    X(4, 1, 10)

#if TINY_REFILL
hipError_t launch_solve_d_refill(const SolveParams &p, hipStream_t stream) {
#define X(NX_, NU_, N_)                                       \
    if (p.nx == NX_ && p.nu == NU_ && p.N == N_)              \
        return p.const_tables ? launch_d_one<NX_, NU_, N_, true>(p, stream) : launch_d_one<NX_, NU_, N_, false>(p, stream);
    TINY_D_SHAPES(X)
#undef X
    return hipErrorInvalidValue;
}
#else
bool solve_d_supported(int nx, int nu, int N, bool const_tables) {
#define X(NX_, NU_, N_) \
    if (nx == NX_ && nu == NU_ && N == N_) return d_vl(NU_, N_, const_tables, d_wpg(NU_, N_, const_tables)) >= 0;
    TINY_D_SHAPES(X)
#undef X
    return false;
}

hipError_t launch_solve_d(const SolveParams &p, hipStream_t stream) {
    if (p.refill_next) return launch_solve_d_refill(p, stream);  // (tinympc_solve_dr.hip)
#define X(NX_, NU_, N_)                                       \
    if (p.nx == NX_ && p.nu == NU_ && p.N == N_)              \
        return p.const_tables ? launch_d_one<NX_, NU_, N_, true>(p, stream) : launch_d_one<NX_, NU_, N_, false>(p, stream);
    TINY_D_SHAPES(X)
#undef X
    return hipErrorInvalidValue;
}

size_t solve_d_lds_bytes(int nu, int N, bool const_tables) {
    const int wpg = d_wpg(nu, N, const_tables);
    return d_lds_bytes(nu, N, const_tables, wpg, d_vl(nu, N, const_tables, wpg));
}

int solve_d_workgroups(int nu, int N, bool const_tables, int groups) {
    const int wpg = d_wpg(nu, N, const_tables);
    return (groups + wpg - 1) / wpg;
}

#endif  // TINY_REFILL

#endif  // TINY_JIT
#endif  // TINY_LEAN

}  // namespace tinympc
