"""The deferred E_in optimizer of cqlrec_train_steps changes no bit.

Inside a call, a row of E_in without a gradient that the NEXT step's forward does not gather is left behind; the launch
that needs it later replays the missed steps in registers (tests/deferred_update_reference.py).  The
last step of a call brings every row up to date.  Strict steps on one stream are the reference; all comparisons are
bitwise on the six raw buffers and the losses, and ctx->grads is all zeros after every call.

Same pattern, helpers, log (U = 2000, window 10, small_log(seed=3, mean_len=14, max_len=45)) and hyper seed (11) as
tests/test_gpu_lean_update.py.  What happens to the rows, from the oracle's sampler on the CPU (B = 256 / B = 128):
    N = 1000, 6 steps   0.63-0.71 / 0.45-0.51 of the rows brought up to date per step, at ages up to 5 (6 steps at once);
    N = 40, 6 steps     every row every step: the deferred form reduces to the lean one;
    N = 5000, 70 steps  0.22-0.25 / 0.13-0.16 of the rows per step; in the (70) call 1251 / 1482 rows are refreshed by the
                        cap alone, 16 / 34 of them are wanted again later in the call, 3 / 15 rows are wanted exactly
                        when they run 64 steps, and 1223 / 1413 rows are wanted by no step before the flush.
"""
import functools

import numpy as np
import pytest
import torch

import deferred_update_reference as R
import test_gpu_lean_update as lean
from test_gpu_lean_update import BUFFERS, L, _assert_same, _log, _pipelined, _strict

pytestmark = pytest.mark.gpu

SEED = 11                      # CQLHyper(seed=11) in lean._core
DB = ((64, 256), (128, 256), (256, 128))
CATALOGUES = {1000: (6, [(6,), (3, 3), (1, 1, 4)]),
              40: (6, [(6,), (3, 3), (1, 1, 4)]),
              5000: (70, [(70,), (64, 6), (1, 69)])}
CASES = [(d, B, Nn, calls) for d, B in DB for Nn, (_, callsets) in CATALOGUES.items() for calls in callsets]


@functools.lru_cache(maxsize=None)
def _reference(d, B, Nn):
    return _strict(d, B, Nn, CATALOGUES[Nn][0])


@functools.lru_cache(maxsize=None)
def _row_sets(B, Nn):
    """(gradient rows, read rows) of the steps 0 .. steps (one more than run: the read map of the step after)"""
    off, items, _ = _log(Nn)
    off, items = np.asarray(off), np.asarray(items)
    sets = [R.sampled_rows(off, items, SEED, t, B, L, Nn) for t in range(CATALOGUES[Nn][0] + 1)]
    return [s[0] for s in sets], [s[1] for s in sets]


def _plans(B, Nn, calls):
    grad, read = _row_sets(B, Nn)
    return R.schedule(grad, read, calls)


@pytest.mark.parametrize("d,B,Nn,calls", CASES)
def test_calls_equal_strict_steps(d, B, Nn, calls):
    """All six buffers and the losses after the calls == the same number of strict steps; grads all zeros after every
    call (checked inside _pipelined); and the next fwd_bwd finds the state and the gradient buffer as good as strict's."""
    ref, ref_grads = _reference(d, B, Nn)
    core, got = _pipelined(d, B, Nn, calls)
    _assert_same(got, ref, calls)
    core.forward_backward(None)
    torch.cuda.synchronize()
    assert torch.equal(core.grads, ref_grads)


@pytest.mark.parametrize("B", [256, 128])
def test_the_catalogues_do_what_they_claim(B):
    """Preconditions of the shapes above, recomputed from the log with the oracle's sampler; the sampler itself is tied to
    the library's through core.views of the last two steps of a call."""
    d = 256 if B == 128 else 128
    for Nn, (steps, callsets) in CATALOGUES.items():
        grad, read = _row_sets(B, Nn)
        assert all((r | ~g).all() for g, r in zip(grad, read))          # windows of s are inside those of s and s'
        for calls in callsets:
            plans = _plans(B, Nn, calls)
            inner = [p for i, p in enumerate(plans) if i not in set(np.cumsum(calls) - 1)]      # steps that do not flush
            shares = [p.processed.mean() for p in inner]
            kmax = max(int(p.k[p.processed].max()) for p in plans)
            if Nn == 40:
                assert all(p.processed.all() and (p.k == 1).all() for p in plans)
            elif Nn == 1000:
                assert all(0.4 < s < 0.8 for s in shares) and not any(p.by_cap.any() for p in plans)
                assert kmax == max(calls)                                 # some row waits for the flush of its call
                assert kmax > 1 or calls == (1,)
            else:
                assert all(0.1 < s < 0.5 for s in shares) and np.mean(shares) < 0.26
                assert kmax == R.CAP
    # N = 5000, one call of 70: cap refreshes, rows wanted again after one, rows wanted exactly at 64, rows nobody wants
    grad, read = _row_sets(B, 5000)
    for calls in ((70,), (1, 69)):
        plans = _plans(B, 5000, calls)
        t0 = 0 if calls == (70,) else 1
        capped = np.zeros(5000, dtype=bool)
        wanted_ever = np.zeros(5000, dtype=bool)
        n_cap = again = at_cap = 0
        for t in range(t0, 69):
            wanted = grad[t] | read[t + 1]
            again += int((capped & wanted).sum())
            at_cap += int((wanted & (plans[t].k == R.CAP)).sum())
            capped = (capped & ~wanted) | plans[t].by_cap
            n_cap += int(plans[t].by_cap.sum())
            wanted_ever |= wanted
        assert n_cap > 1000 and again > 0 and at_cap > 0 and (~wanted_ever).sum() > 1000, (calls, n_cap, again, at_cap)
    assert not any(p.by_cap.any() for p in _plans(B, 5000, (64, 6)))      # there the flush of step 63 comes first
    # the sampler: users / tpos of the last two steps of a pipelined call, as the library drew them
    core, _ = _pipelined(d, B, 1000, (6,))
    off, items, _ = _log(1000)
    off, items = np.asarray(off), np.asarray(items)
    for t in (4, 5):
        v = core.views(t)
        g, r = R.window_rows(off, items, v["users"].cpu().numpy(), v["tpos"].cpu().numpy(), L, 1000)
        assert np.array_equal(g, _row_sets(B, 1000)[0][t]) and np.array_equal(r, _row_sets(B, 1000)[1][t])
        assert np.array_equal(g, lean._touched_rows(core, t, 1000))


@pytest.mark.parametrize("d,B", DB)
def test_stale_rows_are_not_what_the_next_step_reads(d, B):
    """After step k - 1 = 2 of a 6-step call, rows the schedule left behind hold stale bf16 shadows, and step k = 3 gathers
    rows that were brought up to date only because its read map named them.  The state in the middle of a call cannot be
    looked at from outside, so the flush form and the deferred form are compared through what step k makes of them:
    a (k) call, which flushes, equals k strict steps in every row; continuing it, and running the 6 steps as one call,
    give the same loss at step k -- a function of exactly the rows step k reads -- and the same bits from there on."""
    Nn, k, n = 1000, 3, 6
    grad, read = _row_sets(B, Nn)
    plan = _plans(B, Nn, (n,))[k - 1]
    assert (~plan.processed).sum() > 100                                   # rows left behind at the joint ...
    assert (plan.processed & ~grad[k - 1] & (plan.k > 1)).sum() > 0        # ... and rows replayed only for step k's sake
    assert not (read[k] & ~plan.processed).any()
    head_ref, _ = _strict(d, B, Nn, k)
    _, head = _pipelined(d, B, Nn, (k,))
    _assert_same(head, head_ref, (k,))
    _, split = _pipelined(d, B, Nn, (k, n - k))
    _, whole = _pipelined(d, B, Nn, (n,))
    assert torch.equal(whole["losses"][k], split["losses"][k])
    _assert_same(whole, split, "whole vs split")
    ref, _ = _reference(d, B, Nn)
    for nm in BUFFERS:
        assert torch.equal(whole[nm], ref[nm]), nm
