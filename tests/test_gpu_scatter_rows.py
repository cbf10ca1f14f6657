"""The deterministic segmented sums behind both scatters of the step (gbwd.hip), row by row against float64.

Window-gather backward: cqlrec_gather_pool_bwd_sorted and the split form the step driver calls (_prepare + _apply), on
key layouts crafted around the 64-pair chunk edges, on padding that starts mid-chunk / on a chunk edge / fills whole
chunks, on degenerate catalogues, on windows longer than a wave and on shifted (next-state) windows.  One-hot scatter
(cql_onehot_apply, 8-pair chunks, bf16 rows times a weight, accumulate = 1): through the step, on a 40-item catalogue
whose hot actions repeat far beyond a chunk.

Every touched row is held to the element bound (n + 2) u sum |t_i| of scatter_reference.py -- derived, not tuned; the
CPU module test_scatter_reference_cpu.py shows what it accepts and rejects -- and every untouched row to exact zeros."""
import functools

import numpy as np
import pytest
import torch

from oracle import cql_oracle as O
from replay_cql_amd import _native as N
from replay_cql_amd.core import CQLCore, CQLHyper

import scatter_reference as R
from helpers import DEV, bf16_to_np, dev, ptr, stream, sync, ws_bytes_tensor

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return N.load()


@functools.lru_cache(maxsize=None)
def _case(name):
    """(offsets, items, users, ends, end_delta, L, n_items) of a named layout"""
    if name in R.WINDOW_CASES:
        L, delta = R.WINDOW_CASES[name]
        off, items, users, ends, n_items = R.window_case(L, delta)
        return off, items, users, ends, delta, L, n_items
    lay = R.crafted_layout(name)
    off, items, users, ends, L = R.layout_log(lay)
    return off, items, users, ends, 0, L, lay["n_items"]


class _Gather:
    """one layout on the device; g_E_in has n_items + 1 rows (the pad row last), zero-filled before every call"""

    def __init__(self, lib, name, d):
        self.lib, self.d = lib, d
        off, items, users, ends, self.delta, self.L, self.n_items = _case(name)
        self.n = len(users)
        self.host = (off, items, users, ends)
        self.off, self.items, self.users, self.ends = dev(off), dev(items), dev(users), dev(ends)
        self.nb = int(lib.cqlrec_gather_pool_bwd_ws_bytes(self.n, self.L, d))

    def _out(self):
        return torch.zeros((self.n_items + 1, self.d), dtype=torch.float32, device=DEV)

    def sorted(self, dh0):
        g, ws = self._out(), ws_bytes_tensor(self.nb)
        N.check(self.lib.cqlrec_gather_pool_bwd_sorted(ptr(dh0), ptr(self.off), ptr(self.items), ptr(self.users),
                                                       ptr(self.ends), self.delta, self.n, self.L, self.d, self.n_items,
                                                       ptr(ws), self.nb, ptr(g), stream()))
        sync()
        return g

    def split(self, dh0):
        g, ws = self._out(), ws_bytes_tensor(self.nb)
        N.check(self.lib.cqlrec_gather_pool_bwd_prepare(ptr(self.off), ptr(self.items), ptr(self.users), ptr(self.ends),
                                                        self.delta, self.n, self.L, self.d, self.n_items, ptr(ws), self.nb,
                                                        stream()))
        N.check(self.lib.cqlrec_gather_pool_bwd_apply(ptr(dh0), self.n, self.L, self.d, self.n_items, ptr(ws), self.nb,
                                                      ptr(g), stream()))
        sync()
        return g

    def atomic(self, dh0):
        g = self._out()
        N.check(self.lib.cqlrec_gather_pool_bwd(ptr(dh0), ptr(self.off), ptr(self.items), ptr(self.users), ptr(self.ends),
                                                self.delta, self.n, self.L, self.d, ptr(g), stream()))
        sync()
        return g


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("d", [64, 128, 256])
@pytest.mark.parametrize("name", R.CRAFTED + tuple(R.WINDOW_CASES))
def test_gather_bwd_rows(lib, name, d):
    """sorted form == split form == itself again, bit for bit; touched rows inside the element bound; untouched rows and
    the pad row exactly +0.0; on dyadic rows the sorted form equals the atomic scatter exactly"""
    c = _Gather(lib, name, d)
    off, items, users, ends = c.host
    rng = np.random.default_rng(d + len(name))
    dh0 = rng.standard_normal((c.n, d)).astype(np.float32)
    d_dh0 = dev(dh0)
    g = c.sorted(d_dh0)
    assert torch.equal(_bits(c.split(d_dh0)), _bits(g)), "prepare + apply differs from the sorted form"
    assert torch.equal(_bits(c.sorted(d_dh0)), _bits(g)), "two calls differ"
    ref, bound, cnt = R.gather_bwd_reference(dh0, off, items, users, ends, c.delta, c.L, c.n_items)
    got = g.cpu().numpy()
    report = {}
    fails = R.element_check("g_E_in", got[:c.n_items][cnt > 0], ref[cnt > 0], bound[cnt > 0], report)
    print(f"SCATTERCHECK gather_bwd {name} d={d} pairs={c.n * c.L} hottest={int(cnt.max(initial=0))} " + R.fmt_report(report))
    assert not fails, fails
    untouched = np.concatenate([cnt == 0, [True]])
    assert not got.view(np.uint32)[untouched].any(), "a row without pairs (or the pad row) is not +0.0"
    if name == "all_empty":
        assert cnt.sum() == 0 and not got.view(np.uint32).any()
    # dyadic rows: dh0 = len x (multiples of 1/4), so every dh0 / len is a small dyadic number and any order is exact
    _, _, lens = R.window_pairs(off, items, users, ends, c.delta, c.L, c.n_items)
    dy = ((rng.integers(-8, 9, (c.n, d)) / 4.0) * np.maximum(lens, 1)[:, None]).astype(np.float32)
    d_dy = dev(dy)
    gs, ga = c.sorted(d_dy), c.atomic(d_dy)
    assert torch.equal(gs, ga), "sorted form differs from the atomic scatter on dyadic rows"
    ref_dy, _, _ = R.gather_bwd_reference(dy, off, items, users, ends, c.delta, c.L, c.n_items)
    assert np.array_equal(gs.cpu().numpy()[:c.n_items], ref_dy)


# ---- one-hot scatter, through the step ----------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 128, 256])
def test_onehot_scatter_rows_alpha0(d):
    """alpha = 0: the dense kernels contribute 0 x finite, so g_E_out[a] = sum_{act[b] = a} coef[b] hb_s[b] and
    g_b_out[a] = sum coef[b], element by element; rows of actions that were never sampled are exactly zero."""
    OH_N, OH_B, OH_L, OH_SEED = R.OH_N, R.OH_B, R.OH_L, R.OH_SEED
    off, items, rew = R.onehot_case_log()
    m = O.OracleModel.create(OH_N, d, seed=7)
    rng = np.random.default_rng(5)
    for nm in ("b_out", "b1", "b2"):
        m.layout.view(m.theta, nm)[:] = (rng.standard_normal(m.layout.shape(nm)) * 0.05).astype(np.float32)
    m.target[:] = m.theta + (rng.standard_normal(m.theta.shape) * 0.01).astype(np.float32) * (m.theta != 0)
    core = CQLCore(OH_N, CQLHyper(d=d, window=OH_L, batch=OH_B, seed=OH_SEED, alpha=0.0), device=DEV)
    core.load_flat(m.theta, m.target)
    core.set_log(off, items, rew)
    core.forward_backward(None)
    v = core.views()
    act = v["act"].cpu().numpy()
    assert np.array_equal(act, R.onehot_case_actions())
    cnt = np.bincount(act, minlength=OH_N)
    assert R.onehot_case_is_hot(act), cnt              # precondition (test_scatter_reference_cpu.py holds it on the CPU)
    g = core.grads.cpu().numpy()
    lay = m.layout
    gE, gb = lay.view(g, "E_out"), lay.view(g, "b_out")
    refE, boundE, refb, boundb, cnt2 = R.onehot_reference(v["coef"].cpu().numpy(), act, bf16_to_np(v["hb_s"]), OH_N)
    assert np.array_equal(cnt, cnt2)
    report = {}
    fails = R.element_check("g_E_out", gE[cnt > 0], refE[cnt > 0], boundE[cnt > 0], report)
    fails += R.element_check("g_b_out", gb[cnt > 0], refb[cnt > 0], boundb[cnt > 0], report)
    print(f"SCATTERCHECK onehot alpha=0 d={d} hottest={int(cnt.max())} " + R.fmt_report(report))
    assert not fails, fails
    # never sampled: 0 x finite from the dense kernels and nothing else (a nonzero entry here is a finding)
    assert np.all(gE[cnt == 0] == 0) and np.all(gb[cnt == 0] == 0), (gE[cnt == 0], gb[cnt == 0])
    assert np.isfinite(g).all()
    # the same step again gives the same bits
    core2 = CQLCore(OH_N, CQLHyper(d=d, window=OH_L, batch=OH_B, seed=OH_SEED, alpha=0.0), device=DEV)
    core2.load_flat(m.theta, m.target)
    core2.set_log(off, items, rew)
    core2.forward_backward(None)
    torch.cuda.synchronize()
    assert torch.equal(core2.grads.view(torch.int32), core.grads.view(torch.int32))
