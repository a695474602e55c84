// tinympc_lstart_d.hip -- the lean kernels of layout D with the forward steps' accumulator starts read from LDS and the loop control
// out of the lean inner loop (k_admm_solve_d_lean_start, k_admm_solve_d_gbnd_lean_start, launch_solve_d_lean_start): tinympc_solve_d.hip
// with TINY_LEAN and TINY_LEAN_START set. A translation unit of its own, as tinympc_lean_d.hip is: the plain and the lean kernels keep
// their text and with it their code (see the notes at the top of tinympc_solve_d.hip).
#define TINY_LEAN 1
#define TINY_LEAN_START 1
#include "tinympc_solve_d.hip"
