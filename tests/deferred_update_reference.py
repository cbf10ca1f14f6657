"""A numpy model of the deferred E_in optimizer schedule of cqlrec_train_steps.

Inside a call of more than one step, the E_in launch of step t brings a row up to date only if
    the row has a gradient at step t,                                  (window items of s)
    or the forward of step t + 1 gathers it,                           (window items of s and of s')
    or it has fallen CAP - 1 steps behind (this step is its CAP-th),   (the scalar table holds CAP steps)
    or step t is the last of its call.                                 (the flush: callers see complete buffers)
Any other row only has its age -- the number of steps it is behind -- moved on.  A row that is brought up to date runs
`k = age + 1` Adam + Polyak steps, the k - 1 missed ones with g = 0 and then this step's.  Every row is at age 0 when a
call starts; a single-step call is dense.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from oracle import cql_oracle as O

CAP = 64


@dataclass
class StepPlan:
    processed: np.ndarray      # bool [N]: rows the launch of this step brings up to date
    k: np.ndarray              # int  [N]: steps each row runs if processed (its age before the launch + 1)
    by_cap: np.ndarray         # bool [N]: processed for no other reason than the cap


def window_rows(offsets, items, users, tpos, L, n_items):
    """(gradient rows, read rows) of one batch: the items of the windows of s, and those plus the action item (which
    closes the window of s'): items[base - min(tpos, L) .. base) and items[.. base], base = offsets[user] + tpos."""
    grad = np.zeros(n_items, dtype=bool)
    read = np.zeros(n_items, dtype=bool)
    for u, t in zip(np.asarray(users).tolist(), np.asarray(tpos).tolist()):
        base = int(offsets[u]) + t
        lo = base - min(t, L)
        grad[items[lo:base]] = True
        read[items[lo:base + 1]] = True
    return grad, read


def sampled_rows(offsets, items, seed, step, batch, L, n_items):
    """window_rows of the batch the sampler draws for `step` (single rank: slot0 = 0)"""
    pos = O.sample_positions(seed, step, 0, batch, int(offsets[-1]))
    users, tpos = O.positions_to_transitions(pos, np.asarray(offsets))
    return window_rows(offsets, items, users, tpos, L, n_items)


def schedule(grad_rows, read_rows, calls, cap=CAP):
    """grad_rows[t], read_rows[t]: bool [N] for the global steps t = 0 .. sum(calls) - 1; calls: steps per call.
    Returns one StepPlan per step."""
    n_rows = len(grad_rows[0])
    plans, t = [], 0
    for n in calls:
        age = np.zeros(n_rows, dtype=np.int64)
        for i in range(n):
            k = age + 1
            if n == 1 or i == n - 1:
                wanted = np.ones(n_rows, dtype=bool)
            else:
                wanted = grad_rows[t] | read_rows[t + 1]
            processed = wanted | (k >= cap)
            plans.append(StepPlan(processed, k.copy(), processed & ~wanted))
            age = np.where(processed, 0, k)
            t += 1
    return plans
