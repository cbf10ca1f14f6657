"""The deferred E_in schedule replays exactly what the dense optimizer does (CPU, numpy).

`deferred_update_reference.schedule` says which rows the E_in launch of each step brings up to date and how many steps
each of them runs.  Here O.adam_ema_step is applied row-wise along that schedule -- the missed steps with g = 0, each with
the scalars of its own step, then the current one with the row's gradient -- and compared, bit for bit, with the dense
update of every row on every step.  This pins the off-by-ones (age, cap, flush, call boundaries) without a GPU.
"""
import numpy as np
import pytest

from oracle import cql_oracle as O

import deferred_update_reference as R

N_ROWS, D, STEPS, LR = 48, 8, 70, 1e-3
NAMES = ("theta", "m", "v", "target")


def _problem():
    """Row sets in which some rows are wanted every step, some now and then, and some not once in 70 steps; gradient rows
    are read rows of the same step, as windows of s are inside the windows of s and s'."""
    rng = np.random.default_rng(17)
    p_read = np.concatenate([np.full(8, 1.0), np.full(16, 0.3), np.full(8, 0.02), np.full(8, 0.008), np.zeros(8)])
    read = [rng.random(N_ROWS) < p_read for _ in range(STEPS + 1)]
    grad = [r & (rng.random(N_ROWS) < 0.7) for r in read]
    grads = [(rng.standard_normal((N_ROWS, D)) * 0.1).astype(np.float32) * g[:, None] for g in grad]
    state = {"theta": (rng.standard_normal((N_ROWS, D)) * 0.1).astype(np.float32),
             "m": np.zeros((N_ROWS, D), np.float32), "v": np.zeros((N_ROWS, D), np.float32)}
    state["target"] = state["theta"] + (rng.standard_normal((N_ROWS, D)) * 0.01).astype(np.float32)
    return read, grad, grads, state


def _dense(grads, state):
    """state of every row after every step: history[t][name]"""
    cur = {n: state[n].copy() for n in NAMES}
    history = []
    for t in range(STEPS):
        O.adam_ema_step(cur["theta"], grads[t], cur["m"], cur["v"], cur["target"], t + 1, LR)
        history.append({n: cur[n].copy() for n in NAMES})
    return history


@pytest.fixture(scope="module")
def problem():
    read, grad, grads, state = _problem()
    return read, grad, grads, state, _dense(grads, state)


@pytest.mark.parametrize("calls", [(70,), (64, 6), (1, 69)])
def test_schedule_replays_the_dense_update(problem, calls):
    read, grad, grads, state, dense = problem
    plans = R.schedule(grad, read, calls)
    assert len(plans) == STEPS
    cur = {n: state[n].copy() for n in NAMES}
    behind = np.zeros(N_ROWS, dtype=np.int64)          # tracked here, independently of the plan's k
    call_ends = set(np.cumsum(calls) - 1)
    seen_k = set()
    for t, plan in enumerate(plans):
        assert np.array_equal(plan.k, behind + 1)
        assert plan.k.max() <= R.CAP                   # the scalar table holds CAP steps
        if t + 1 < STEPS and t not in call_ends:
            assert plan.processed[read[t + 1]].all()   # what the next forward gathers is up to date
        assert plan.processed[grad[t]].all()
        rows = np.flatnonzero(plan.processed)
        for r in rows:
            k = int(plan.k[r])
            seen_k.add(k)
            row = [cur[n][r] for n in NAMES]
            zero = np.zeros(D, np.float32)
            for a in range(k - 1, -1, -1):             # oldest missed step first
                O.adam_ema_step(row[0], grads[t][r] if a == 0 else zero, row[1], row[2], row[3], t - a + 1, LR)
            for a in range(1, k):                      # a skipped step had no gradient
                assert not grad[t - a][r]
        for n in NAMES:                                # a processed row holds the dense state of THIS step ...
            assert np.array_equal(cur[n][rows], dense[t][n][rows]), (calls, t, n)
        behind = np.where(plan.processed, 0, behind + 1)
        if t in call_ends:                             # ... and after the flush every row does
            assert plan.processed.all()
            for n in NAMES:
                assert np.array_equal(cur[n], dense[t][n]), (calls, t, n)
    assert max(seen_k) == R.CAP                        # a row nobody wants runs CAP steps at once, never more
    if calls != (64, 6):                               # (in (64, 6) it is the flush of step 63 that gets there first)
        assert any(p.by_cap.any() for p in plans)
    assert {2, 3, 5} <= seen_k


def test_every_dense_row_step_is_accounted_for(problem):
    """The steps the schedule runs, replayed ones included, are exactly the N x STEPS row-steps of the dense form."""
    read, grad, _, _, _ = problem
    for calls in ((70,), (64, 6), (1, 69)):
        plans = R.schedule(grad, read, calls)
        done = np.zeros((STEPS, N_ROWS), dtype=np.int64)
        for t, plan in enumerate(plans):
            for r in np.flatnonzero(plan.processed):
                done[t - int(plan.k[r]) + 1:t + 1, r] += 1
        assert (done == 1).all()


def test_single_step_calls_are_dense(problem):
    read, grad, _, _, _ = problem
    plans = R.schedule(grad[:3], read[:4], (1, 1, 1))
    assert all(p.processed.all() and (p.k == 1).all() for p in plans)


def test_window_rows_are_the_windows_of_s_and_s_prime():
    offsets = np.array([0, 4, 9])
    items = np.array([5, 6, 7, 8, 1, 2, 3, 4, 0])
    grad, read = R.window_rows(offsets, items, users=[0, 1], tpos=[0, 4], L=3, n_items=10)
    assert np.flatnonzero(grad).tolist() == [2, 3, 4]               # user 1: items[5..8) = 2 3 4; user 0 at tpos 0: none
    assert np.flatnonzero(read).tolist() == [0, 2, 3, 4, 5]         # + the action items 5 (user 0) and 0 (user 1)
