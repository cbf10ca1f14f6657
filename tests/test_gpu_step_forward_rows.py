"""The forward half of the training step through CQLCore, against float64 rows and exact bits -- the forms only the
step launches (cql_qhead_argmax_step forces the QM_ARGMAX skeleton at d = 128; cqlrec_qhead_fwd never runs it there).

  test                                   what it pins
  test_dyadic_forward_bit_exact_shapes   h0, h, Q(s, a), arg-max, Q_target as bits at d = 64 / 128 / 256 (one to 32 slices)
  test_step_argmax_ties                  the smallest index wins at every boundary of the arg-max geometry: the skeleton
                                         at d = 128 (64-item stages, 32 slices of 192), qargmax2 at d = 256 (32-item
                                         stages by register-set parity, 8 slices of 576)
  test_step_forward_rows                 random model, every reference from the step's OWN views and bf16 shadows: lse rows
                                         inside bound_lse, q_a and q_targ as the bits of gather_dot, a_star by the derived
                                         margin rule, y and coef by the TD kernel's element bound"""
import numpy as np
import pytest
import torch

from oracle import cql_oracle as O
from replay_cql_amd.core import CQLCore, CQLHyper

import pairs_reference as PR
import qhead_forward_reference as R
import scatter_reference as SR
from helpers import DEV, bf16_to_np, small_log

pytestmark = pytest.mark.gpu


def _make(U, Nn, d, B, L, dyadic=False):
    off, items, rew = small_log(U=U, N=Nn, seed=3, mean_len=14, max_len=45)
    m = O.OracleModel.create(Nn, d, seed=7, dyadic=dyadic)
    rng = np.random.default_rng(5)
    if not dyadic:
        for nm in ("b_out", "b1", "b2"):
            m.layout.view(m.theta, nm)[:] = (rng.standard_normal(m.layout.shape(nm)) * 0.05).astype(np.float32)
        m.target[:] = m.theta + (rng.standard_normal(m.theta.shape) * 0.01).astype(np.float32) * (m.theta != 0)
    core = CQLCore(Nn, CQLHyper(d=d, window=L, batch=B, seed=11, alpha=1.0), device=DEV)
    core.load_flat(m.theta, m.target)
    core.set_log(off, items, rew)
    return m, core, (off, items, rew)


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _u32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("B", [32, 96, 256])
@pytest.mark.parametrize("Nn", [40, 513, 4099])
@pytest.mark.parametrize("d", [64, 128, 256])
def test_dyadic_forward_bit_exact_shapes(d, Nn, B):
    L = 4
    m, core, (off, items, rew) = _make(80, Nn, d, B, L, dyadic=True)
    core.forward_backward(None)
    v = core.views()
    pos = O.sample_positions(11, 0, 0, B, int(off[-1]))
    users, tpos = O.positions_to_transitions(pos, off)
    out = O.loss_and_grads(m.layout, m.theta, m.target, off, items, rew, users, tpos, L, 0.99, 1.0)
    assert np.array_equal(_u32(v["h0_s"].cpu().numpy()), _u32(out.h0_s))
    assert np.array_equal(_u32(bf16_to_np(v["hb_s"])), _u32(out.hb_s))
    assert np.array_equal(_u32(bf16_to_np(v["hb_sn"])), _u32(out.hb_sn))
    # Q(s, a), Q_target: the model is dyadic, the STATE VECTORS are not (bf16 roundings of an MLP's output), so a score is
    # exact in fp32 -- and the oracle's fp32 dot product THE value -- only on rows whose d + 1 terms share a quantum that
    # 24 bits span (_exact_rows).  There the oracle's bits are required (most rows at d = 64, about a tenth at d = 256;
    # against the oracle's bits on all rows 14 of the 27 shapes differ in some row).  On EVERY row
    # the bits of the kernel's own operation order are required (pairs_reference.gather_dot from the step's views), and
    # the oracle's value inside the any-order fp32 bound of the row.
    E_t, E_g = _bits(core.segment(core.theta_b, "E_out")), _bits(core.segment(core.target_b, "E_out"))
    b_t, b_g = core.segment(core.theta, "b_out").cpu().numpy(), core.segment(core.target, "b_out").cpu().numpy()
    act, a_star = v["act"].cpu().numpy(), v["a_star"].cpu().numpy()
    n_exact = 0
    for name, hb, Eb, bb, it, ref in (("q_a", _bits(v["hb_s"]), E_t, b_t, act, out.q_a),
                                      ("q_targ", _bits(v["hb_tn"]), E_g, b_g, a_star, out.q_targ)):
        got = v[name].cpu().numpy()
        assert np.array_equal(_u32(got), _u32(PR.gather_dot(hb, Eb, bb, np.arange(B), it))), name
        exact, bound = _exact_rows(hb, Eb, bb, it)
        n_exact += int(exact.sum())
        assert np.array_equal(_u32(got[exact]), _u32(ref[exact])), name
        assert (np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= 2 * bound).all(), name
    print(f"ROWCHECK step-forward dyadic d={d} N={Nn} B={B} exact_rows={n_exact}/{2 * B}")
    # a*: the oracle's on every row whose two best exact scores are further apart than their fp32 bounds; the derived
    # margin rule on all rows (the scores of a near-tie are not exact in fp32, see above)
    H_n, E_f = PR.bf16_bits_to_f32(_bits(v["hb_sn"])), PR.bf16_bits_to_f32(E_t)
    R.check_argmax(H_n, E_f, b_t, a_star)
    clear = np.zeros(B, bool)
    for lo, hi, S, e in R.scores64(H_n, E_f, b_t):
        top2 = np.argsort(-S, axis=1, kind="stable")[:, :2]
        r = np.arange(hi - lo)
        clear[lo:hi] = S[r, top2[:, 0]] - S[r, top2[:, 1]] > 2 * (e[r, top2[:, 0]] + e[r, top2[:, 1]])
    assert clear.any() and np.array_equal(a_star[clear], out.a_star[clear])


def _exact_rows(hb_bits, E_bits, b, items):
    """(mask of the pairs whose score is exact in fp32 IN ANY ORDER, the any-order bound (d + 1) u sum |t| of every pair):
    with A = sum |terms| < 2^k every partial sum is below 2^k, and exact when every term is a multiple of 2^(k - 24)"""
    h = PR.bf16_bits_to_f32(hb_bits).astype(np.float64)
    e = PR.bf16_bits_to_f32(E_bits).astype(np.float64)[np.asarray(items, np.int64)]
    t = np.concatenate([h * e, np.asarray(b, np.float64)[np.asarray(items, np.int64)][:, None]], 1)
    A = np.abs(t).sum(1)
    g = 2.0 ** (np.ceil(np.log2(np.maximum(A, 1e-300))) + 1 - 24)
    q = t / g[:, None]
    return (q == np.round(q)).all(1), (t.shape[1]) * R.U32 * A


@pytest.mark.parametrize("d", [128, 256])
def test_step_argmax_ties(d):
    Nn, B, L = 4099, 64, 5
    form, stage, nsplit, split_rows = R.argmax_geometry(d, B, Nn, step=True)
    assert (form, stage) == (("skeleton", 64) if d == 128 else ("qargmax2", 32)) and nsplit >= 2 and split_rows < Nn
    m, core, _ = _make(64, Nn, d, B, L, dyadic=True)
    lay = m.layout
    positions = sorted({x for fg in R.tie_positions(stage, 32, split_rows, Nn, parity=(d == 256)) for x in fg})
    assert 0 in positions and Nn - 1 in positions and split_rows in positions and split_rows - 1 in positions
    for f in positions:
        theta = m.theta.copy()
        lay.view(theta, "E_out")[:] = lay.view(m.theta, "E_out")[0]
        bo = lay.view(theta, "b_out")
        bo[:] = 0.25
        bo[f:] += 1.0                       # a dyadic step: items f.. share the maximum on every row
        core.load_flat(theta, theta)
        core.forward_backward(None)
        a_star = core.views()["a_star"].cpu().numpy()
        assert (a_star == f).all(), (f, a_star[:8])


@pytest.mark.parametrize("U,Nn,d,B,L", [(64, 257, 64, 64, 5), (300, 1000, 128, 256, 8), (200, 4099, 128, 96, 50),
                                        (100, 513, 256, 128, 10), (64, 40, 128, 256, 5), (64, 65, 128, 32, 5)])
def test_step_forward_rows(U, Nn, d, B, L):
    m, core, _ = _make(U, Nn, d, B, L)
    core.forward_backward(None)
    v = core.views()
    E_t, E_g = _bits(core.segment(core.theta_b, "E_out")), _bits(core.segment(core.target_b, "E_out"))
    b_t, b_g = core.segment(core.theta, "b_out").cpu().numpy(), core.segment(core.target, "b_out").cpu().numpy()
    hb_s, hb_sn, hb_tn = _bits(v["hb_s"]), _bits(v["hb_sn"]), _bits(v["hb_tn"])
    act, a_star = v["act"].cpu().numpy(), v["a_star"].cpu().numpy()
    rows = np.arange(B)
    report = {}
    # lse: the fused forward of the step, rows = B
    first = R.fused_form(d, Nn)
    ref = R.LseReference(PR.bf16_bits_to_f32(hb_s), PR.bf16_bits_to_f32(E_t), b_t, R.lse_forms(B, Nn, d))
    name = "fused_generic" if first == "generic" else first
    assert first == "generic" or not ref.overflow[first]
    report["lse"] = R.check_lse(v["lse"].cpu().numpy(), ref, name)
    # Q(s, a) and the double-Q target: bits
    assert np.array_equal(_u32(v["q_a"].cpu().numpy()), _u32(PR.gather_dot(hb_s, E_t, b_t, rows, act))), "q_a"
    assert np.array_equal(_u32(v["q_targ"].cpu().numpy()), _u32(PR.gather_dot(hb_tn, E_g, b_g, rows, a_star))), "q_targ"
    # a*: the derived margin rule on the online network's scores of s'
    R.check_argmax(PR.bf16_bits_to_f32(hb_sn), PR.bf16_bits_to_f32(E_t), b_t, a_star)
    # y and coef: the TD kernel's element bound, from the step's own q_a, lse, q_targ
    td = SR.td_reference(v["q_a"].cpu().numpy(), v["lse"].cpu().numpy(), v["q_targ"].cpu().numpy(), v["rew"].cpu().numpy(),
                         v["done"].cpu().numpy(), 0.99, 1.0, np.float32(1.0) / np.float32(B))
    fails = SR.element_check("y", v["y"].cpu().numpy(), *td["y"], report)
    fails += SR.element_check("coef", v["coef"].cpu().numpy(), *td["coef"], report)
    print(f"ROWCHECK step-forward {name} B={B} N={Nn} d={d} " + SR.fmt_report(report))
    assert not fails, fails
