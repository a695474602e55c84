// tinympc_lshare_d.hip -- the trimmed lean kernels of layout D with d and the slack sharing the register slots in the lean inner loop
// (k_admm_solve_d_lean_share, k_admm_solve_d_gbnd_lean_share, launch_solve_d_lean_share): tinympc_solve_d.hip with TINY_LEAN,
// TINY_LEAN_START, TINY_LEAN_TRIM and TINY_LEAN_SHARE set. A translation unit of its own, as tinympc_lean_d.hip, tinympc_lstart_d.hip and
// tinympc_ltrim_d.hip are: the plain, the lean, the lean-start and the trimmed kernels keep their text and with it their code (see the
// notes at the top of tinympc_solve_d.hip). (The file's name does not start with tinympc_solve: tests/test_isa_hazards.py keeps a list of
// those.)
#define TINY_LEAN 1
#define TINY_LEAN_START 1
#define TINY_LEAN_TRIM 1
#define TINY_LEAN_SHARE 1
#include "tinympc_solve_d.hip"
