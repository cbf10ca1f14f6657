"""CPU self-test of the row-wise softmax-gradient checker (helpers.softmax_grad_rows): what justifies its K.

GPU-like results are made in numpy the way the kernels make them -- P = exp2 of an fp32 argument, rounded to bf16 at
the true scale (item side) or relative to per-slice references and rescaled afterwards (fused forward), products summed
in fp32 in a different order, the one-hot term added in fp32 -- and must be ACCEPTED.  Each fault a kernel could make
in the dense term must be REJECTED, with the faulty row named."""
import numpy as np
import pytest

from oracle import cql_oracle as O

from helpers import ROWS_K, softmax_grad_reference, softmax_grad_rows

LOG2E = np.float32(1.4426950408889634)


def _case(B, Nn, d, kind, seed):
    """Operands as the training step has them: bf16 states with peaked (large norm) and flat (small norm) softmax rows
    in one batch, bf16 item table, fp32 bias, the fp32 lse a kernel would produce, a realistic coef, actions with
    duplicates.  kind "coherent": 63 of 64 states tiny, as at initialisation -- P[b, j] is nearly the same for all states
    b, so the bf16 rounding errors of an item row's terms are nearly equal and add up instead of averaging out."""
    rng = np.random.default_rng(seed)
    amp = rng.choice([0.05, 0.5, 3.0, 8.0], size=B).astype(np.float32)
    if kind == "coherent":
        amp[np.arange(B) % 64 != 0] = 0.01
    H = O.bf16_round(rng.standard_normal((B, d)).astype(np.float32) * amp[:, None])
    E = O.bf16_round((rng.standard_normal((Nn, d)) / np.sqrt(d)).astype(np.float32))
    b = (rng.standard_normal(Nn) * 0.3).astype(np.float32)
    Q = H.astype(np.float64) @ E.T.astype(np.float64) + b
    m = Q.max(1)
    lse = (m + np.log(np.exp(Q - m[:, None]).sum(1))).astype(np.float32)
    delta = rng.standard_normal(B).astype(np.float32)
    coef = ((delta - np.float32(1.0)) / np.float32(B)).astype(np.float32)
    act = rng.integers(0, Nn, B).astype(np.int64)
    act[: min(B, 6)] = act[0]
    return dict(H=H, E=E, b=b, lse=lse, coef=coef, act=act, scale=np.float32(1.0 / B), Q=Q)


def _p32(c, ref_shift=None):
    """fp32 P as the kernels form it: exp2(fma(S + b, log2e, -ref log2e)), ref = lse (true scale) or a shifted
    reference (fused forward)."""
    S = (c["H"] @ c["E"].T + c["b"]).astype(np.float32)           # fp32 scores (sgemm: its own summation order)
    ref = c["lse"] if ref_shift is None else ref_shift
    return np.exp2(S * LOG2E - (ref * LOG2E).astype(np.float32)[:, None]).astype(np.float32)


def _chain(blocks):
    """fp32 sum of per-block fp32 partials, one block after the other (a long accumulator chain)."""
    acc = np.zeros_like(blocks[0])
    for x in blocks:
        acc = (acc + x).astype(np.float32)
    return acc


def _dense_true_scale(c, P, order):
    Pb = O.bf16_round(P)
    H, E = c["H"], c["E"]
    if order == "sgemm":
        return Pb.T @ H, P.sum(0, dtype=np.float32), Pb @ E
    # chains of 32-term MFMA blocks: over the states in reverse order (item side), over the items (state side)
    B, Nn = P.shape
    dE = _chain([Pb[lo:lo + 32].T @ H[lo:lo + 32] for lo in reversed(range(0, B, 32))])
    db = _chain([P[lo:lo + 32].sum(0, dtype=np.float32) for lo in reversed(range(0, B, 32))])
    dH = _chain([Pb[:, lo:lo + 32] @ E[lo:lo + 32] for lo in range(0, Nn, 32)])
    return dE, db, dH


def _dh_shifted(c, seed):
    """Fused forward: two item slices, each with a per-state reference of its own (slice maximum + 0..8 nats), P rounded
    to bf16 relative to it, the slices merged with exp(ref - lse) afterwards."""
    rng = np.random.default_rng(seed)
    Nn = c["E"].shape[0]
    cut = max(1, Nn // 2)
    out = np.zeros((c["H"].shape[0], c["E"].shape[1]), dtype=np.float32)
    S = (c["H"] @ c["E"].T + c["b"]).astype(np.float32)
    for lo, hi in ((0, cut), (cut, Nn)):
        if hi <= lo:
            continue
        ref = (S[:, lo:hi].max(1) + rng.uniform(0, 8, S.shape[0])).astype(np.float32)
        Pr = np.exp2(S[:, lo:hi] * LOG2E - (ref * LOG2E)[:, None]).astype(np.float32)
        part = O.bf16_round(Pr) @ c["E"][lo:hi]
        w = np.exp2(ref * LOG2E - c["lse"] * LOG2E).astype(np.float32)
        out = (out + w[:, None] * part).astype(np.float32)
    return out


def _with_onehot(c, dE, db, dH):
    """The kernels' outputs: scale * dense in fp32, one-hot term added in fp32 (one rounding per addition)."""
    sc = c["scale"]
    gE, gb, gH = (sc * dE).astype(np.float32), (sc * db).astype(np.float32), (sc * dH).astype(np.float32)
    if c.get("with_coef", True):
        np.add.at(gE, c["act"], c["coef"][:, None] * c["H"])
        np.add.at(gb, c["act"], c["coef"])
        gH = (gH + c["coef"][:, None] * c["E"][c["act"]]).astype(np.float32)
    return gE, gb, gH


def _check(c, ref, gE, gb, gH):
    kw = dict(coef=c["coef"], act=c["act"]) if c.get("with_coef", True) else {}
    return softmax_grad_rows(c["H"], c["lse"], c["E"], c["b"], c["scale"], g_E_out=gE, g_b_out=gb, dH=gH, ref=ref, **kw)


CASES = [(5, 37, 64, "mixed"), (1024, 20011, 64, "mixed"), (1024, 8005, 128, "mixed"), (1024, 4001, 256, "mixed"),
         (1024, 3001, 128, "coherent")]


@pytest.fixture(scope="module", params=CASES, ids=lambda p: "B%d_N%d_d%d_%s" % p)
def case(request):
    B, Nn, d, kind = request.param
    c = _case(B, Nn, d, kind, seed=B + Nn + d)
    ref = softmax_grad_reference(c["H"], c["lse"], c["E"], c["b"], c["scale"])
    P = _p32(c)
    return c, ref, P


@pytest.mark.parametrize("with_coef", [False, True])
@pytest.mark.parametrize("variant", ["true_scale_sgemm", "true_scale_chained", "shifted_scale"])
def test_checker_accepts_gpu_like_rounding(case, variant, with_coef):
    c, ref, P = case
    c = dict(c, with_coef=with_coef)
    if variant == "shifted_scale":
        dE, db, _ = _dense_true_scale(c, P, "sgemm")
        dH = _dh_shifted(c, seed=3)
    else:
        dE, db, dH = _dense_true_scale(c, P, variant.split("_")[-1])
    rep = _check(c, ref, *_with_onehot(c, dE, db, dH))
    # headroom under K: a row made of one dominant term reaches 2 (the largest bf16 rounding error is 2^-8 = 2 sigma);
    # rows of many terms stay near 1 (their errors add up like a Gaussian of deviation sigma)
    assert max(rep.values()) < 0.6 * ROWS_K, rep


FAULTS = ["group_zeroed", "last_partial_group_dropped", "rows_swapped_in_tile", "last_33_states_missing",
          "lse_of_neighbour_row", "dh_row_softmax_zeroed", "db_group_missing"]


@pytest.mark.parametrize("fault", FAULTS)
def test_checker_rejects_fault(case, fault):
    c, ref, P = case
    B, Nn = P.shape
    dE, db, dH = (x.astype(np.float32) for x in _dense_true_scale(c, P, "sgemm"))
    Pb = O.bf16_round(P)
    g = min(1, (Nn - 1) // 256)                       # an item group that exists (and is whole when possible)
    if fault == "group_zeroed":
        dE[256 * g: 256 * (g + 1)] = 0
        expect = "/256:%d" % g
    elif fault == "last_partial_group_dropped":
        lo = Nn // 256 * 256
        assert lo < Nn
        dE[lo:] = 0
        db[lo:] = 0
        expect = "/256:%d" % (Nn // 256)
    elif fault == "rows_swapped_in_tile":
        j0 = 32 * ((Nn // 2) // 32)
        r1, r2 = j0 + 5, min(Nn - 1, j0 + 20)
        dE[[r1, r2]] = dE[[r2, r1]]
        expect = "g_E_out"
    elif fault == "last_33_states_missing":
        k = min(33, B - 1)
        dE -= Pb[B - k:].T @ c["H"][B - k:]
        db -= P[B - k:].sum(0, dtype=np.float32)
        expect = "g_E_out"
    elif fault == "lse_of_neighbour_row":
        r = int(np.argmax(np.abs(np.diff(c["lse"]))))                      # a row whose neighbour's lse differs
        assert abs(float(c["lse"][r] - c["lse"][r + 1])) > 1e-2
        P_wrong = np.exp2(((c["Q"][r] * LOG2E).astype(np.float32) - c["lse"][r + 1] * LOG2E)).astype(np.float32)
        dH[r] = O.bf16_round(P_wrong) @ c["E"]
        dE += np.outer(O.bf16_round(P_wrong) - Pb[r], c["H"][r])
        db += P_wrong - P[r]
        expect = "dH: 1 of"
    elif fault == "dh_row_softmax_zeroed":
        r = B // 2
        dH[r] = 0
        expect = "dH: 1 of"
    elif fault == "db_group_missing":
        db[256 * g: 256 * (g + 1)] = 0
        expect = "g_b_out"
    with pytest.raises(AssertionError) as ei:
        _check(c, ref, *_with_onehot(c, dE, db, dH))
    assert expect in str(ei.value), str(ei.value)
