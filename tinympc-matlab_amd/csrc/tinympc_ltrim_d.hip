// tinympc_ltrim_d.hip -- the lean-start kernels of layout D with the instructions beside the arithmetic trimmed out of the lean inner loop
// (k_admm_solve_d_lean_trim, k_admm_solve_d_gbnd_lean_trim, launch_solve_d_lean_trim): tinympc_solve_d.hip with TINY_LEAN, TINY_LEAN_START
// and TINY_LEAN_TRIM set. A translation unit of its own, as tinympc_lean_d.hip and tinympc_lstart_d.hip are: the plain, the lean and the
// lean-start kernels keep their text and with it their code (see the notes at the top of tinympc_solve_d.hip).
#define TINY_LEAN 1
#define TINY_LEAN_START 1
#define TINY_LEAN_TRIM 1
#include "tinympc_solve_d.hip"
