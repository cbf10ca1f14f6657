"""CPU self-test of the scatter reference (scatter_reference.py): what justifies the element bound of the GPU row tests.

A NumPy fp32 port of the two-pass segmented sum (gbwd.hip), chunk length a parameter, is run in the kernel's order, in
reverse order and with pairwise pieces over every key layout of test_gpu_scatter_rows.py, and must stay INSIDE the bound
(n + 2) u sum |t_i| against float64.  Each fault a rewrite of the kernels could make -- a term dropped, a term added
twice, an edge piece credited to the neighbouring key, a padding pair summed into the last row -- must be REJECTED by
the same bound, on a hot run (640 pairs) and on a run of two."""
import numpy as np
import pytest

from oracle import cql_oracle as O

import scatter_reference as R

D = 8            # row width of the emulation: the bound is per element, the width only multiplies the work
ORDERS = ("kernel", "reverse", "pairwise")


def _case(name):
    """sorted (keys, vals), lens, n_items of a named layout"""
    if name.startswith("L"):
        L, delta = R.WINDOW_CASES[name]
        off, items, users, ends, n_items = R.window_case(L, delta)
    else:
        lay = R.crafted_layout(name)
        off, items, users, ends, L = R.layout_log(lay)
        n_items, delta = lay["n_items"], 0
    keys, vals, lens = R.window_pairs(off, items, users, ends, delta, L, n_items)
    ks, vs = R.sorted_pairs(keys, vals)
    return ks, vs, lens, n_items


def _terms(vs, lens, seed=0):
    """fp32 terms g[state] = dh0[state] / len as gbwd_scale_kernel forms them, and the float64 terms of the reference"""
    rng = np.random.default_rng(seed)
    dh0 = rng.standard_normal((lens.size, D)).astype(np.float32)
    ln = np.maximum(lens, 1)
    g32 = (dh0 / ln[:, None].astype(np.float32)).astype(np.float32)
    return g32[vs], dh0.astype(np.float64)[vs] / ln[vs][:, None]


LAYOUTS = R.CRAFTED + ("L70", "L50d1")


def test_crafted_layouts_are_what_they_claim():
    """run ends at 64q - 1, 64q, 64q + 1; whole-chunk runs; the edge-crossing pair; where the padding starts; idle waves"""
    ks, _, _, n_items = _case("runs")
    lay = R.crafted_layout("runs")
    last = np.cumsum(R.RUN_COUNTS) - 1
    first = last - np.array(R.RUN_COUNTS) + 1
    assert {63, 127, 191, 319, 575, 639} <= set(last[last % 64 == 63]) and {128, 384, 576, 2304} <= set(last[last % 64 == 0])
    assert 577 in last[last % 64 == 1]
    whole = [(f, c) for f, c in zip(first, R.RUN_COUNTS) if f % 64 == 0 and c % 64 == 0]
    assert {c // 64 for _, c in whole} >= {1, 2, 10}
    assert first[R.PAIR_RUN] % 64 == 63 and R.RUN_COUNTS[R.PAIR_RUN] == 2
    assert np.array_equal(ks, np.repeat(lay["run_ids"], R.RUN_COUNTS))
    assert np.setdiff1d(np.arange(n_items), lay["run_ids"]).size >= 5          # item ids that get no pair
    geo = {nm: R.segsum_geometry(_case(nm)[0], _case(nm)[3], 64) for nm in R.CRAFTED}
    assert (geo["runs"]["live"], geo["runs"]["idle_waves"]) == (2310, 3)
    assert (geo["pad_mid"]["live"], geo["pad_mid"]["idle_waves"], geo["pad_mid"]["pad_chunks"]) == (2310, 1, 2)
    assert geo["pad_mid"]["live"] % 64 != 0
    assert (geo["pad_edge"]["live"], geo["pad_edge"]["idle_waves"]) == (2304, 2) and geo["pad_edge"]["pad_chunks"] == 2
    assert geo["all_empty"]["live"] == 0
    assert geo["one_item"]["live"] == 663 and _case("one_item")[3] == 1


@pytest.mark.parametrize("ch", [64, 8, 5])
@pytest.mark.parametrize("name", LAYOUTS)
def test_emulation_stays_inside_the_bound(name, ch):
    ks, vs, lens, n_items = _case(name)
    t32, t64 = _terms(vs, lens)
    ref, ab, cnt = R.segsum_reference(ks, t64, n_items)
    bound = R.sum_bound(cnt[:, None], ab)
    report, fails = {}, []
    for order in ORDERS:
        got = R.segsum_emulate(ks, t32, n_items, n_items, ch, order)
        fails += R.element_check(order, got[:n_items], ref, bound, report)
        assert not got[n_items].any(), "the pad row was written"
        assert not got[:n_items][cnt == 0].any(), "a row without pairs was written"
    print(f"SCATTERCHECK emulation {name} ch={ch} " + R.fmt_report(report))
    assert not fails, fails


def test_emulation_orders_differ():
    """the three orders are different fp32 computations (otherwise the test above checks one order three times)"""
    ks, vs, lens, n_items = _case("runs")
    t32, _ = _terms(vs, lens)
    outs = [R.segsum_emulate(ks, t32, n_items, n_items, 64, o) for o in ORDERS]
    assert not np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[0], outs[2])


def _fault_case(victim):
    """sorted pairs of a layout with 40 padding pairs in which the hot run / the run of two is ALSO the last item id:
    (keys, terms32, ref, bound, n_items, victim key, a pair of the victim, a padding pair)"""
    counts = list(R.RUN_COUNTS)
    if victim == "hot":                      # a 640-run that starts mid-chunk, moved to the end
        counts = counts[:15] + counts[16:] + [640]
    else:                                    # the run of two that crosses the edge 2303 | 2304, last
        counts = counts[:18]
    keys = np.repeat(np.arange(len(counts)), counts)
    n_items = len(counts)
    start = keys.size - counts[-1]
    assert start // 64 != (keys.size - 1) // 64, "the victim run must cross a chunk edge"
    ks = np.concatenate([keys, np.full(40, n_items)])
    rng = np.random.default_rng(5)
    t32 = rng.standard_normal((ks.size, D)).astype(np.float32)
    ref, ab, cnt = R.segsum_reference(ks, t32.astype(np.float64), n_items)
    return ks, t32, ref, R.sum_bound(cnt[:, None], ab), n_items, n_items - 1, start + 1, keys.size + 7


@pytest.mark.parametrize("ch", [64, 8])
@pytest.mark.parametrize("victim", ["hot", "pair"])
def test_planted_faults_are_rejected(victim, ch):
    ks, t32, ref, bound, n_items, key, pair, pad_pair = _fault_case(victim)
    if ch == 8 and victim == "pair":
        # the run of two sits at 2303 | 2304: an edge of the 8-pair chunks as well
        assert (pair - 1) // 8 != pair // 8
    clean = R.segsum_emulate(ks, t32, n_items, n_items, ch)
    assert not R.element_check("clean", clean[:n_items], ref, bound, {})
    for fault in (("drop", pair), ("twice", pair), ("edge_to_neighbour", key), ("pad_into_last", pad_pair)):
        got = R.segsum_emulate(ks, t32, n_items, n_items, ch, fault=fault)
        rep = {}
        fails = R.element_check(fault[0], got[:n_items], ref, bound, rep)
        assert fails, f"{fault} on the {victim} run slipped through (worst ratio {rep})"
        assert f"({key}, " in fails[0] or fault[0] == "edge_to_neighbour", fails      # the victim's row is named
        print(f"SCATTERCHECK fault {fault[0]} {victim} ch={ch} " + R.fmt_report(rep))


def test_onehot_case_is_hot():
    """precondition of test_gpu_scatter_rows.py::test_onehot_scatter_rows_alpha0, from the sampler's oracle alone"""
    act = R.onehot_case_actions()
    cnt = np.bincount(act, minlength=R.OH_N)
    assert R.onehot_case_is_hot(act), cnt
    assert (cnt >= 9).sum() >= 3 and cnt.max() > 64 and (cnt == 0).any(), cnt
    # the catalogue / batch pair is the lean-update module's
    from helpers import small_log
    ref = small_log(U=R.OH_U, N=R.OH_N, seed=3, mean_len=14, max_len=45)
    assert all(np.array_equal(a, b) for a, b in zip(ref, R.onehot_case_log()))


def test_element_check_is_strict():
    """exact where the bound is zero, NaN never passes, the worst ratio is what is reported"""
    ref = np.array([[1.0, 0.0]])
    bound = np.array([[1e-7, 0.0]])
    assert not R.element_check("x", np.array([[1.0 + 5e-8, 0.0]]), ref, bound, {})
    assert R.element_check("x", np.array([[1.0, 1e-45]]), ref, bound, {})
    assert R.element_check("x", np.array([[np.nan, 0.0]]), ref, bound, {})
    rep = {}
    assert R.element_check("x", np.array([[1.0 + 3e-7, 0.0]]), ref, bound, rep) and abs(rep["x"] - 3.0) < 1e-6


def test_encoder_and_td_references_accept_fp32_and_reject_faults():
    """the propagated bounds hold for a plain fp32 evaluation (another order than the kernels': BLAS) and still see one
    row counted twice / a dead row left alive / the done mask dropped"""
    rng = np.random.default_rng(2)
    rows, d = 129, 64
    dH = rng.standard_normal((rows, d)).astype(np.float32)
    zb = O.bf16_round(np.maximum(rng.standard_normal((rows, d)), 0).astype(np.float32))
    zb[::8] = 0
    h0b = O.bf16_round(rng.standard_normal((rows, d)).astype(np.float32))
    W1b = O.bf16_round((rng.standard_normal((d, d)) / np.sqrt(d)).astype(np.float32))
    W2b = O.bf16_round((rng.standard_normal((d, d)) / np.sqrt(d)).astype(np.float32))
    ref, dead = R.encoder_bwd_reference(dH, zb, h0b, W1b, W2b)
    assert dead[::8].all()
    dA1 = ((dH @ W2b) * (zb > 0)).astype(np.float32)
    got = {"dh0": dA1 @ W1b, "gW1": dA1.T @ h0b, "gb1": dA1.sum(0, dtype=np.float32), "gW2": dH.T @ zb,
           "gb2": dH.sum(0, dtype=np.float32)}
    rep, fails = {}, []
    for nm, (r, b) in ref.items():
        fails += R.element_check(nm, got[nm], r, b, rep)
    print("SCATTERCHECK encoder fp32 " + R.fmt_report(rep))
    assert not fails, fails
    twice = (dA1.T @ h0b + np.outer(dA1[5], h0b[5])).astype(np.float32)
    assert R.element_check("gW1", twice, *ref["gW1"], {})
    alive = ((dH @ W2b).astype(np.float32) @ W1b)              # relu mask dropped
    assert R.element_check("dh0", alive, *ref["dh0"], {})
    # TD
    B = 257
    q_a, lse, qt, rew = [rng.standard_normal(B).astype(np.float32) for _ in range(4)]
    lse = (lse + 5).astype(np.float32)
    done = (rng.random(B) < 0.3).astype(np.float32)
    g, a, inv = np.float32(0.99), np.float32(0.7), np.float32(1.0 / (2 * B))
    td = R.td_reference(q_a, lse, qt, rew, done, g, a, inv)
    y = rew + g * (np.float32(1) - done) * qt
    delta = q_a - y
    coef = (delta - a) * inv
    loss = np.float32((np.float32(0.5) * delta * delta + a * (lse - q_a)).sum(dtype=np.float32) * inv)
    rep = {}
    fails = R.element_check("y", y, *td["y"], rep) + R.element_check("coef", coef, *td["coef"], rep) + \
        R.element_check("loss", np.array(loss), *td["loss"], rep)
    print("SCATTERCHECK td fp32 " + R.fmt_report(rep))
    assert not fails, fails
    y_bad = rew + g * qt                                          # done mask dropped
    assert R.element_check("y", y_bad, *td["y"], {})
