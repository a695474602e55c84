// tinympc_rollout_noise.h -- the one draw behind the rollout's process and measurement noise (tinympc_set_rollout_noise; k_plant_step's
// noisy variants and k_rollout_noise, tinympc_rollout.hip). Counter-based: a draw is a pure function of
//     (seed, g, tick, r, stream)     g: the instance's global index (first_instance + b), tick: the handle's noise tick, r: the state row,
//                                     stream: 0 process noise, 1 measurement noise
// -- no generator state, no upload, no kernel of its own per tick; independent of the layout, of W and KT, of how a rollout is cut into
// calls and of how a fleet is cut into handles.
//   generator  Philox4x32-10 (Salmon et al., SC'11; the Random123 constants): counter (g, tick, r, stream), key (seed & 0xffffffff,
//              seed >> 32), multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85; output words o0..o3.
//   uniforms   u1 = ((o0 >> 5) 2^26 + (o1 >> 6) + 1) 2^-53 in (0, 1],  u2 = ((o2 >> 5) 2^26 + (o3 >> 6)) 2^-53 in [0, 1): 53 bits each,
//              exact in float64.
//   normal     n = sqrt(-2 log(u1)) * cos(6.283185307179586 * u2)  (Box-Muller, one of the pair): every operation rounded once, nothing
//              contracted. |n| <= sqrt(106 ln 2) = 8.58.
#pragma once
#include <hip/hip_runtime.h>

namespace tinympc {

__device__ __forceinline__ double rollout_normal(unsigned k0, unsigned k1, unsigned g, unsigned tick, unsigned r, unsigned stream) {
#pragma clang fp contract(off)
    unsigned c0 = g, c1 = tick, c2 = r, c3 = stream;
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (unsigned)p1; c2 = n2; c3 = (unsigned)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    const double u1 = (double)(((unsigned long long)(c0 >> 5) << 26) + (c1 >> 6) + 1) * 0x1p-53;
    const double u2 = (double)(((unsigned long long)(c2 >> 5) << 26) + (c3 >> 6)) * 0x1p-53;
    const double radius = sqrt(-2.0 * log(u1));
    const double angle = 6.283185307179586 * u2;
    return radius * cos(angle);
}

}  // namespace tinympc
