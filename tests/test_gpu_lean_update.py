"""The lean optimizer launches of cqlrec_train_steps change no bit.

Inside one cqlrec_train_steps call, a step that has a successor leaves ctx->grads un-zeroed: the item-side range is
overwritten by the next long dE_out kernel, and the E_in range is read through a per-row "touched this step" map (rows
the batch did not touch take g = 0 without being read, so what an earlier step left in them is dead).  The last step
of a call clears everything.  All comparisons here are bitwise on the raw buffers.

Shapes: U = 2000, window 10, B = 256 (128 for d = 256), three catalogues --
    N = 1000   rows touched in some steps and not in others (the stale-row case lives here),
    N = 40     every row touched every step (the map is all ones),
    N = 5000   most rows never touched.
None of the three is a multiple of the item group (256 items; 128 for d = 256), so each has a partial last group.
Cut groups (CqlAdamFix.valid, qhead_de.hip: some block range p * W / grid starts inside a group, W = G x T stage-units,
grid = min(W, CUs)): at these sizes W < 256 CUs, so grid = W, every block owns ONE stage-unit, and with T = B / 64 = 4
(d = 64, 128) or T = B / 32 = 4 (d = 256, B = 128) three of the four stages of EVERY group are cut pieces that go to
slabs -- N = 40 (G = 1, W = 4) is already the smallest catalogue that sets the flag, all nine shapes have it set.
"""
import functools
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import cql_oracle as O
from replay_cql_amd import _native as N
from replay_cql_amd.core import CQLCore, CQLHyper

from helpers import DEV, small_log

pytestmark = pytest.mark.gpu

U, L, STEPS = 2000, 10, 5
BUFFERS = ("theta", "adam_m", "adam_v", "target", "theta_b", "target_b")
SHAPES = [(d, B, Nn) for d, B in ((64, 256), (128, 256), (256, 128)) for Nn in (1000, 40, 5000)]


@functools.lru_cache(maxsize=None)
def _log(Nn):
    return small_log(U=U, N=Nn, seed=3, mean_len=14, max_len=45)


@functools.lru_cache(maxsize=None)
def _model(Nn, d):
    m = O.OracleModel.create(Nn, d, seed=7)
    rng = np.random.default_rng(5)
    for nm in ("b_out", "b1", "b2"):
        m.layout.view(m.theta, nm)[:] = (rng.standard_normal(m.layout.shape(nm)) * 0.05).astype(np.float32)
    m.target[:] = m.theta + (rng.standard_normal(m.theta.shape) * 0.01).astype(np.float32) * (m.theta != 0)
    return m


def _core(d, B, Nn):
    m = _model(Nn, d)
    core = CQLCore(Nn, CQLHyper(d=d, window=L, batch=B, seed=11), device=DEV)
    core.load_flat(m.theta, m.target)
    core.set_log(*_log(Nn))
    return core


def _snapshot(core, losses):
    torch.cuda.synchronize()
    snap = {n: getattr(core, n).clone() for n in BUFFERS}
    snap["losses"] = losses.clone()
    return snap


def _assert_same(got, ref, what):
    for n in BUFFERS + ("losses",):
        assert torch.equal(got[n], ref[n]), (what, n)


def _grads_are_zero(core):
    torch.cuda.synchronize()
    return torch.count_nonzero(core.grads.view(torch.int32)).item() == 0      # bit pattern: -0.0 would count


def _strict(d, B, Nn, steps):
    """`steps` strict steps (fwd_bwd + update, one stream, program order) on a fresh core, then one more fwd_bwd whose
    gradient is kept: (state after `steps` steps, gradient of step `steps`)."""
    core = _core(d, B, Nn)
    losses = torch.zeros(steps, device=DEV)
    N.check(N.load().cqlrec_set_concurrency(0))
    try:
        for i in range(steps):
            core.forward_backward(losses[i:i + 1])
            core.apply_update()
        snap = _snapshot(core, losses)
        core.forward_backward(None)
        torch.cuda.synchronize()
        grads = core.grads.clone()
    finally:
        N.check(N.load().cqlrec_set_concurrency(1))
    return snap, grads


@functools.lru_cache(maxsize=None)
def _reference(d, B, Nn):
    return _strict(d, B, Nn, STEPS)


def _pipelined(d, B, Nn, calls):
    """the calls one after another on a fresh core; grads must be all zeros after each"""
    core = _core(d, B, Nn)
    losses = torch.zeros(sum(calls), device=DEV)
    done = 0
    for n in calls:
        core.train_steps(n, losses[done:])
        done += n
        assert _grads_are_zero(core), (calls, done)
    return core, _snapshot(core, losses)


@pytest.mark.parametrize("d,B,Nn", SHAPES)
def test_one_call_equals_strict_steps(d, B, Nn):
    """One call of 5 pipelined steps (4 lean + the clearing last one) == 5 strict steps, in all six buffers and the
    losses; grads all zeros afterwards; and the next fwd_bwd finds the gradient buffer as good as freshly zeroed."""
    ref, ref_grads = _reference(d, B, Nn)
    core, got = _pipelined(d, B, Nn, (STEPS,))
    _assert_same(got, ref, "5")
    core.forward_backward(None)
    torch.cuda.synchronize()
    assert torch.equal(core.grads, ref_grads)


@pytest.mark.parametrize("calls", [(3, 2), (1, 1, 3)])
@pytest.mark.parametrize("d,B,Nn", SHAPES)
def test_split_calls_equal_one_call(d, B, Nn, calls):
    """The last step of every call clears; the row maps restart by parity at an odd and at an even step0; a single-step
    call takes the full form."""
    ref, ref_grads = _reference(d, B, Nn)
    core, got = _pipelined(d, B, Nn, calls)
    _assert_same(got, ref, calls)
    core.forward_backward(None)
    torch.cuda.synchronize()
    assert torch.equal(core.grads, ref_grads)


def _touched_rows(core, step, Nn):
    """E_in rows the window-gather backward of `step` writes: the items of the sampled windows (gbwd_pairs_kernel)"""
    v = core.views(step)
    users, tpos = v["users"].cpu().numpy(), v["tpos"].cpu().numpy()
    off, items, _ = _log(Nn)
    off, items = np.asarray(off), np.asarray(items)
    rows = np.zeros(Nn, dtype=bool)
    for u, end in zip(users, tpos):
        ln = min(int(end), L)
        rows[items[off[u] + end - ln: off[u] + end]] = True
    return rows


def test_catalogue_extremes_are_what_they_claim():
    """N = 40: the map is all ones; N = 5000: most rows are never touched (preconditions of the shapes above)."""
    core, _ = _pipelined(128, 256, 40, (STEPS,))
    assert _touched_rows(core, STEPS - 1, 40).all() and _touched_rows(core, STEPS - 2, 40).all()
    core, _ = _pipelined(128, 256, 5000, (STEPS,))
    assert (_touched_rows(core, STEPS - 1, 5000) | _touched_rows(core, STEPS - 2, 5000)).mean() < 0.5


@pytest.mark.parametrize("t_next_is_last", [True, False])
def test_row_touched_then_untouched(t_next_is_last):
    """A row touched at step t = 3 and untouched at t + 1 = 4 holds a stale gradient when step 4's optimizer runs.
    t + 1 last in its call (5 steps): the clearing form must take it as zero AND clear it.  t + 1 with a successor
    (6 steps): the lean form must not read it.  Either way the state equals the strict twin's."""
    d, B, Nn = 128, 256, 1000
    steps = 5 if t_next_is_last else 6
    core, got = _pipelined(d, B, Nn, (steps,))
    # (views of the last two steps stay addressable by parity; for the 6-step call re-run 5 to look at steps 3 and 4)
    look = core if t_next_is_last else _pipelined(d, B, Nn, (5,))[0]
    at_t, at_next = _touched_rows(look, 3, Nn), _touched_rows(look, 4, Nn)
    stale = np.flatnonzero(at_t & ~at_next)
    assert stale.size > 0
    ref = _reference(d, B, Nn)[0] if t_next_is_last else _strict(d, B, Nn, steps)[0]
    _assert_same(got, ref, steps)
    lay = core.layout
    r0 = int(lay.off_E_in) + int(stale[0]) * d
    assert torch.equal(got["adam_m"][r0:r0 + d], ref["adam_m"][r0:r0 + d])
    assert torch.count_nonzero(core.grads[r0:r0 + d].view(torch.int32)).item() == 0


def test_late_item_side_kernel_gives_the_same_bits():
    """CQL_EARLY_DE=0 puts the long item-side kernel behind the loss instead of behind the fused forward: it still
    overwrites every row before anyone reads one.  The knob is read once per process: two fresh child processes."""
    root = Path(__file__).resolve().parents[1]
    outs = []
    for knob in ("1", "0"):
        env = dict(os.environ, CQL_EARLY_DE=knob)
        cmd = [sys.executable, str(root / "tools" / "train_digest.py"), "--d", "128", "--items", "1000", "--users", "2000",
               "--batch", "256", "--steps", "4"]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    assert outs[0]["losses"] == outs[1]["losses"]
    assert outs[0]["state_sha256"] == outs[1]["state_sha256"]
