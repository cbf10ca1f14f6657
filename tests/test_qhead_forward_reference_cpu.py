"""CPU self-test of tests/qhead_forward_reference.py: what justifies using its bound on the GPU.

* An fp32 port of the lse pipeline (fp32 scores, per-slice (reference, sum) partials, the merge of
  qhead_finalize_lse_kernel) in three summation orders must stay INSIDE bound_lse at every GPU-test shape with N <= 5003.
* On the flat rows every fault a kernel could make with ONE item or ONE partial must fall OUTSIDE it.
* The condition that makes the second point possible -- on flat rows the smallest probability is at least 4 bound_lse -- is
  asserted for every "none"-bias input of the GPU module, the largest N included.  (A ramp bias is not flat by design and
  a +200 step makes the QM_LSE form's own legitimate error proportional to 200 u per tile: there one item of 20011 is
  below what ANY fp32 kernel of that form resolves, so those inputs carry no such condition.)
* The ports of the split functions against values worked out from the C++ by hand; the tie enumerator on the three
  geometries in use."""
import numpy as np
import pytest

import qhead_forward_reference as R

LSE_SHAPES = [(1, 5), (1, 33), (32, 64), (33, 65), (255, 257), (257, 4099), (300, 5003), (1024, 20011)]
DIMS = (64, 128, 256)


forms_of = R.lse_forms


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("B,Nn", LSE_SHAPES)
def test_flat_rows_can_see_one_item(B, Nn, d):
    H, E, b, flat = R.lse_inputs(B, Nn, d, "none")
    assert flat[0]
    rows = np.nonzero(flat)[0][:8]                     # the bound of a flat row depends on N and d, hardly on the row
    ref = R.LseReference(H[rows], E, b, forms_of(B, Nn, d))
    for name, bd in ref.bound.items():
        assert (ref.pmin >= 4.0 * bd).all(), (name, float(ref.pmin.min()), float(bd.max()))


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("B,Nn", [s for s in LSE_SHAPES if s[1] <= 5003])
@pytest.mark.parametrize("bias", ["none", "ramp"])
def test_fp32_pipeline_stays_inside_the_bound(B, Nn, d, bias):
    H, E, b, _ = R.lse_inputs(B, Nn, d, bias)
    H = H[:48]                                         # the slice geometry is that of the full batch
    forms = forms_of(B, Nn, d)
    ref = R.LseReference(H, E, b, forms)
    worst = {}
    for name, form in forms.items():
        if ref.overflow[name]:
            continue
        for order in ("sgemm", "chain16", "reverse"):
            lse, nlse2 = R.lse_emulate(H, E, b, form, order)
            worst[name] = max(worst.get(name, 0.0), R.check_lse(lse, ref, name))
            assert np.array_equal(nlse2, (-lse * R.LOG2E32).astype(np.float32))
    assert worst and max(worst.values()) <= 1.0, worst


def _mutations(H, E, b, form, row_a, row_b):
    """name -> float32 lse of every row after the fault (float64 arithmetic: only the fault separates it from the reference)"""
    Nn = E.shape[0]
    out = {}

    def lse_of(Hx, Ex, bx, weights=None):
        for _, _, S, _ in R.scores64(Hx, Ex, bx, block=1 << 20):
            m = S.max(1)
            w = np.ones(S.shape[1]) if weights is None else weights
            return (m + np.log((np.exp(S - m[:, None]) * w).sum(1))).astype(np.float32)
    j = Nn // 2
    w = np.ones(Nn)
    w[j] = 0.0
    out["one item dropped"] = lse_of(H, E, b, w)
    w = np.ones(Nn)
    w[j] = 2.0
    out["one item counted twice"] = lse_of(H, E, b, w)
    out["a padding item counted with bias 0"] = lse_of(H, np.vstack([E, np.zeros((1, E.shape[1]), np.float32)]),
                                                      np.append(b, np.float32(0)))
    if form.nsplit >= 2:
        w = np.ones(Nn)
        w[form.slice_of == form.nsplit - 1] = 0.0
        out["one slice's partial dropped"] = lse_of(H, E, b, w)
    good = lse_of(H, E, b)
    if abs(float(good[row_a]) - float(good[row_b])) > 0:
        sw = good.copy()
        sw[[row_a, row_b]] = sw[[row_b, row_a]]
        out["two rows swapped"] = sw
    if Nn % 32 > 1:
        E2, b2 = E.copy(), b.copy()
        E2[Nn - 1], b2[Nn - 1] = E[Nn - 2], b[Nn - 2]
        out["the last item of a partial tile replaced by its neighbour"] = lse_of(H, E2, b2)
    return out


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("B,Nn", [(33, 65), (257, 4099), (300, 5003), (1024, 20011)])
def test_bound_rejects_one_item_faults(B, Nn, d):
    H, E, b, flat = R.lse_inputs(B, Nn, d, "none")
    fl = np.nonzero(flat)[0][:4]
    pk = np.nonzero(~flat)[0]
    # peaked rows on which the last item weighs most (its score against the row's lse ~ ln N + |h|^2 / 2 d)
    pk = pk[np.argsort(-(H[pk] @ E[Nn - 1] - (H[pk] ** 2).sum(1) / (2 * d)))][:28]
    rows = np.concatenate([fl, pk])                    # flat rows first
    assert len(fl) >= 2 and len(pk) >= 8
    forms = forms_of(B, Nn, d)
    ref = R.LseReference(H[rows], E, b, forms)
    for name, form in forms.items():
        muts = _mutations(H[rows], E, b, form, 0, len(fl))          # the swap: a flat row with a peaked one
        assert len(muts) >= (6 if form.nsplit >= 2 and Nn % 32 > 1 else 4), list(muts)
        for what, lse in muts.items():
            if what == "two rows swapped":
                for r in (0, len(fl)):
                    with pytest.raises(AssertionError):
                        R.check_lse(lse[r: r + 1], ref, name, rows=np.array([r]))
            elif what == "the last item of a partial tile replaced by its neighbour":
                # moves a row by p_last (exp(s_neighbour - s_last) - 1): nothing on a flat row, whose items score alike
                # (that row cannot tell the two items apart by construction); the peaked rows of the same batch see it
                with pytest.raises(AssertionError):
                    R.check_lse(lse, ref, name)
            else:
                for r in range(len(fl)):               # every flat row on its own
                    with pytest.raises(AssertionError):
                        R.check_lse(lse[r: r + 1], ref, name, rows=np.array([r]))


def test_split_ports():
    # qargmax2: rblks = 2, units = 65, want = min(128, 65 // 8 = 8) = 8, upb = 9
    assert R.qargmax2_split(257, 4099) == (8, 576)
    # one row-block: want = min(256, 8): the same slices
    assert R.qargmax2_split(1, 4099) == (8, 576)
    # fewer than 16 units (960 = 15 x 64): units // 8 = 1, one slice
    assert R.qargmax2_split(256, 960) == (1, 960)
    # 8 stages x 2 slices: units = 16 -> want 2, upb 8
    assert R.qargmax2_split(256, 1024) == (2, 512)
    # forward skeleton: rblks = 1, units = 65, want = 768 -> max_split 32 -> 32, upb = 3
    assert R.fwd_split(96, 4099) == (22, 192)
    # a catalogue of one unit: one slice
    assert R.fwd_split(1, 5) == (1, 64)
    # rows = 1024: rblks = 4, want = 192 -> max_split 156 -> rounded to 160 -> capped 156, upb = ceil(313 / 156) = 3
    assert R.fwd_split(1024, 20011) == (105, 192)
    # fused forward: rows = 300 -> rblks = 3, target 512 -> want 171 -> max_split 32 -> 32; upb = 3
    assert R.fused_split(300, 4099, 128) == (22, 192)
    # qfwd3 halves the target: rblks = 8 -> want 32, units 313, upb = 10
    assert R.fused_split(1024, 20011, 256) == (32, 640)
    assert R.fused_form(64, 4099) == "generic" and R.fused_form(128, 4099) == "qfwd2" and R.fused_form(256, 4099) == "qfwd3"
    assert R.argmax_geometry(128, 64, 4099, step=True)[0] == "skeleton"
    assert R.argmax_geometry(128, 64, 4099)[0] == "qargmax2" and R.argmax_geometry(64, 64, 4099)[0] == "skeleton"
    assert R.argmax_geometry(256, 64, 4099, step=True) == ("qargmax2", 32, 8, 576)


def test_tie_positions():
    # 64-item stages with two tiles (qargmax2 at d = 128), slices of 576
    p = R.tie_positions(64, 32, 576, 4099)
    assert p == [(0, 1), (3, 4), (31, 32), (63, 64), (575, 576), (0, 4098), (4097, 4098)]
    # 32-item stages with one tile (qargmax2 at d = 256): the parity positions
    p = R.tie_positions(32, 32, 576, 4099, parity=True)
    assert p == [(0, 1), (3, 4), (31, 32), (575, 576), (0, 4098), (4097, 4098), (63, 64), (127, 128), (95, 96)]
    # the 64-item skeleton on a catalogue of one slice: positions past N drop out
    assert R.tie_positions(64, 32, 64, 33) == [(0, 1), (3, 4), (31, 32), (0, 32)]
    for pattern in R.TIE_PATTERNS:
        H, E, b = R.dyadic_inputs(5, 70, 64, 1)
        for f, g in R.tie_positions(64, 32, 64, 70):
            E2, b2, want = R.tie_layout(E, b, pattern, f, g)
            idx, val = R.exact_argmax(H, E2, b2)
            assert (idx == want).all(), (pattern, f, g)


def test_argmax_rule_rejects_a_wrong_item():
    H, E, b, _ = R.lse_inputs(33, 65, 64, "none")
    S = next(R.scores64(H, E, b))[2]
    idx = S.argmax(1)
    val = S.max(1).astype(np.float32)
    assert R.check_argmax(H, E, b, idx, val) <= 1.0
    second = np.argsort(-S, axis=1)[:, 1]
    peaked = int(np.argmax(S.max(1) - S[np.arange(33), second]))
    wrong = idx.copy()
    wrong[peaked] = second[peaked]
    with pytest.raises(AssertionError):
        R.check_argmax(H, E, b, wrong, val)
    with pytest.raises(AssertionError):
        R.check_argmax(H, E, b, idx, val + np.float32(1e-3))
