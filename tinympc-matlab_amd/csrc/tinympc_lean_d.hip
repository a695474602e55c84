// tinympc_lean_d.hip -- the lean variant of layout D's compiled-in kernels (k_admm_solve_d_lean, k_admm_solve_d_gbnd_lean,
// launch_solve_d_lean): tinympc_solve_d.hip with TINY_LEAN set. A translation unit of its own so that the plain kernels' text -- and
// with it their code -- is exactly what it is without the variant (see the notes at the top of tinympc_solve_d.hip).
#define TINY_LEAN 1
#include "tinympc_solve_d.hip"
