// tinympc_lpark_d.hip -- the shared lean kernels of layout D with a second slot split that holds only inside a run of lean rounds
// (k_admm_solve_d_lean_park, k_admm_solve_d_gbnd_lean_park, launch_solve_d_lean_park): tinympc_solve_d.hip with TINY_LEAN,
// TINY_LEAN_START, TINY_LEAN_TRIM, TINY_LEAN_SHARE and TINY_LEAN_PARK set. A translation unit of its own, as tinympc_lean_d.hip,
// tinympc_lstart_d.hip, tinympc_ltrim_d.hip and tinympc_lshare_d.hip are: the plain, the lean, the lean-start, the trimmed and the shared
// kernels keep their text and with it their code (see the notes at the top of tinympc_solve_d.hip). Quadrotor N=50 only: the shapes
// without LDS slots have nothing to convert. (The file's name does not start with tinympc_solve: tests/test_isa_hazards.py keeps a list
// of those.)
#define TINY_LEAN 1
#define TINY_LEAN_START 1
#define TINY_LEAN_TRIM 1
#define TINY_LEAN_SHARE 1
#define TINY_LEAN_PARK 1
#include "tinympc_solve_d.hip"
