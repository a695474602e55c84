"""The rollout noise's draw restated in numpy (include/tinympc_hip.h, tinympc_set_rollout_noise): Philox4x32-10 in integer arithmetic, the
two 53-bit uniforms, and the normal in float64 in the documented order -- log, times -2, sqrt, the angle's product, cos, the last product,
one numpy operation each --, vectorised over whatever shape the counters have. The integer part is exact; the normal differs from the
device's by what the two math libraries' log and cos differ (a few ulp)."""
from __future__ import annotations

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox(counter, key):
    """counter: four arrays (or integers) of 32-bit values, key: two. Returns the four output words as uint64 arrays holding 32-bit values."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in np.broadcast_arrays(*counter)]
    k = [int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]  # 32 x 32 bits: exact in 64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k[0]), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k[1]), p0 & MASK]
        k = [(k[0] + W0) & 0xFFFFFFFF, (k[1] + W1) & 0xFFFFFFFF]
    return c


def uniforms(words):
    """u1 in (0, 1], u2 in [0, 1): 53 bits each, exact in float64."""
    o = [np.asarray(w, dtype=np.uint64) for w in words]
    n1 = (o[0] >> np.uint64(5)) * np.uint64(1 << 26) + (o[1] >> np.uint64(6)) + np.uint64(1)
    n2 = (o[2] >> np.uint64(5)) * np.uint64(1 << 26) + (o[3] >> np.uint64(6))
    return n1.astype(np.float64) * 2.0 ** -53, n2.astype(np.float64) * 2.0 ** -53


def normal(seed, g, tick, r, stream):
    """n(g, tick, r, stream) for the 64-bit seed; the counters broadcast against each other."""
    seed = int(seed)
    u1, u2 = uniforms(philox((g, tick, r, stream), (seed & 0xFFFFFFFF, seed >> 32)))
    radius = np.sqrt(-2.0 * np.log(u1))
    angle = 6.283185307179586 * u2
    return radius * np.cos(angle)


def terms(seed, scales, stream, nx, first_tick, ticks, batch, first_instance=0):
    """What the steps add: scale_r * n, (nx, ticks, batch) in the disturbance's layout. scales: (nx,) or (nx, batch), or None (zeros)."""
    if scales is None:
        return np.zeros((nx, ticks, batch))
    s = np.asarray(scales, dtype=np.float64)
    s = s[:, None, None] if s.ndim == 1 else s[:, None, :]
    r = np.arange(nx, dtype=np.uint64)[:, None, None]
    t = (np.uint64(first_tick) + np.arange(ticks, dtype=np.uint64))[None, :, None]
    g = (np.uint64(first_instance) + np.arange(batch, dtype=np.uint64))[None, None, :]
    return s * normal(seed, g, t, r, stream)
