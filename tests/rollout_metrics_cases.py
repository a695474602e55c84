"""The rollout metrics restated in numpy (include/tinympc_hip.h, tinympc_set_rollout_metrics): the eight slots of every instance from a
rollout's own logs, the references and bounds its solves used at knot 0, and the weights. The cost is summed the documented way -- one
chain per step from the value so far, one term per row, state rows ascending, then input rows ascending, every product rounded once
(e e, then times the weight) -- in float64 operations numpy performs one at a time (vectorised over the batch only: each instance's
chain is sequential), so the result is the library's bit for bit."""
from __future__ import annotations

import numpy as np

NAMES = ("steps", "cost", "x_violation", "u_violation", "iterations", "max_iterations", "unconverged", "settle")


def restate(x_log, u_log, iter_log, status_log, xr, ur, x_bounds, u_bounds, qx, ru, settle_tol, start=None):
    """x_log (nx, >= ticks, batch), u_log (nu, ticks, batch), iter_log / status_log (ticks, batch): a rollout's logs. xr (nx, ticks, batch),
    ur (nu, ticks, batch): knot 0 of the reference of every step's solve. x_bounds / u_bounds: (lo, hi), each (rows, batch) -- knot 0 of
    the bounds --, or None while that family is off. qx (nx,), ru (nu,), settle_tol. start: rows to continue from (batch, 8), default
    zeros. Returns (batch, 8) float64."""
    x_log, u_log = np.asarray(x_log, dtype=np.float64), np.asarray(u_log, dtype=np.float64)
    nx, nu = x_log.shape[0], u_log.shape[0]
    ticks, batch = u_log.shape[1], u_log.shape[2]
    rows = np.zeros((batch, 8)) if start is None else np.array(start, dtype=np.float64)
    for t in range(ticks):
        x, u = x_log[:, t, :], u_log[:, t, :]
        e, d = x - xr[:, t, :], u - ur[:, t, :]
        cost = rows[:, 1].copy()
        for i in range(nx):
            sq = e[i] * e[i]
            cost = cost + qx[i] * sq
        for j in range(nu):
            sq = d[j] * d[j]
            cost = cost + ru[j] * sq
        rows[:, 0] += 1.0
        rows[:, 1] = cost
        if x_bounds is not None:
            lo, hi = x_bounds
            rows[:, 2] = np.fmax(rows[:, 2], np.fmax(0.0, np.fmax(lo - x, x - hi)).max(axis=0))
        if u_bounds is not None:
            lo, hi = u_bounds
            rows[:, 3] = np.fmax(rows[:, 3], np.fmax(0.0, np.fmax(lo - u, u - hi)).max(axis=0))
        it = np.asarray(iter_log[t], dtype=np.float64)
        rows[:, 4] += it
        rows[:, 5] = np.fmax(rows[:, 5], it)
        rows[:, 6] += (np.asarray(status_log[t]) != 1)  # (anything but TINYMPC_STATUS_SOLVED: a tick out of iterations reports 11)
        if settle_tol > 0.0:
            away = np.abs(e).max(axis=0) > settle_tol
            rows[:, 7] = np.where(away, rows[:, 0], rows[:, 7])
    return rows


def as_rows(metrics):
    """The dict of rollout_metrics() as (batch, 8) float64, slot order."""
    return np.stack([np.asarray(metrics[k], dtype=np.float64) for k in NAMES], axis=1)
