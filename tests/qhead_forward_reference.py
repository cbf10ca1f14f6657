"""Float64 reference and DERIVED bounds for the Q-head forward (logsumexp, arg-max, scores), NumPy ports of the host-side
split functions, and crafted tie layouts.  NumPy only: the CPU self-test (test_qhead_forward_reference_cpu.py) and the GPU
modules (test_gpu_qhead_forward_rows.py, test_gpu_step_forward_rows.py) share it.

Exact scores.  H, E are bf16 values, b is fp32: a product of two bf16 values has 16 significant bits and is exact in
float64, and the float64 sum of d <= 256 of them plus b errs by < 2^-44 of the sum of magnitudes -- 2^-20 of any fp32
effect.  scores64 is "the" score.

Score bound e_j = (d + 1) c u (|b_j| + sum_k |h_k| |e_jk|), u = 2^-24, c = C_MFMA = 2.
  The kernels form a score as a chain of d / 16 MFMAs (v_mfma_f32_32x32x16_bf16), the bias as C operand of the first:
  d + 1 exact terms, d additions.  For additions rounded to nearest IN ANY ORDER the classical bound is
  d u sum |t| (1 + O(d u)); (d + 1) absorbs the higher-order terms (helpers.topk_certificate uses that bound, c = 1).
  The ISA does not specify the matrix pipe's internal order NOR the rounding of its intermediate sums: an implementation
  may align the 16 products and C to the largest exponent and truncate.  The weakest property under which it still is an
  fp32 accumulation is that every one of the d additions is FAITHFUL: it errs by less than one ulp = 2 u of its result,
  instead of u for round-to-nearest.  That doubles the classical bound and nothing else: c = 2.  (A tree instead of a
  chain, or a wider internal accumulator, only lowers the error.)

lse bound of one row, for the exact scores s, softmax p, computed scores s^ with |s^_j - s_j| <= e_j:
  bound = exp(2 max e) sum_j p_j e_j            lse is 1-Lipschitz along p: d lse / d s_j = p_j; p moves by <= exp(2 max e)
        + u sum_j p_j rel_j  (+ its square)     relative error of item j's term of the sum L, see below; -log(1 - x) <= x + x^2
        + 6 u |log L|                           logf: 3 ulp = 6 u |result| (no fast-math; the weakest documented guarantee of
                                                the OpenCL-derived device library's log; the hardware instruction
                                                underneath, v_log_f32, is stated as 1 ulp by the ISA guide)
        + u |lse|                               the final ms + logf(L)
  rel_j, in units of u, per form (FORM_* below; derived from qhead.hip / qhead_fwd2.hip / qhead_fwd3.hip).  Shared pieces:
    E1  exp2(fma(x, log2e, fl(-r log2e))): the fma result rounds (u |x - r| log2e, in base-2 units), fl(-r log2e)
        rounds (u |r| log2e), the fp32 constant log2e is off by < u relative (u |x - r| log2e); times ln 2 that is a
        relative error of P of u (2 |x - r| + |r|); v_exp_f32 adds 1 ulp = 2 u (ISA guide: "1 ULP"; the guides of this
        project give no figure, so the ISA's is used).             E1(x, r) = 2 |x - r| + |r| + 2
    E2  w = exp2(fl(fl(x - r) log2e)), then fl(w t): difference, product, constant, exp2, product:
                                                                   E2(x, r) = 3 |x - r| + 3
    depth_j: the number of fp32 additions the term passes through: <= 17 inside its tile (16 terms of the lane, then the
        running sum), one per later tile of its slice, one for the lane pair, one per slice in the finalize kernel from
        its own on.  A sum of positive terms errs by at most (number of additions a term passes) u, relative, per term.
    With M the row maximum, a_j = M - s_j, R_j = max(|M|, |s_j|):
    FORM_LSE (QM_LSE skeleton; the reference is the lane's running maximum r, s_j <= r <= M, no margin): the term is formed
        by E1 with |x - r| <= a_j, |r| <= R_j; EVERY later tile of the slice multiplies the running sum by
        exp2(fma(st_a, log2e, off)) -- an E1 whose |x - r| telescope to <= a_j over the chain and whose |r| <= R_j each
        time, plus the product (the factor is not exactly 1 even when the maximum did not move: the fma keeps the
        rounding residual of M log2e against fl(M log2e), up to u |M| log2e); the lane-pair merge and the
        finalize kernel are one E2 each with |x - r| <= a_j:
            rel_j = 10 a_j + (1 + T_j) R_j + 3 T_j + 8 + depth_j          T_j = later tiles of j's slice
    FORM_FUSED (QM_LSE_DH skeleton, also the guarded fall-back; running reference r = tile maximum + QS_REF_MARGIN when
        beaten, so s_j <= r <= M + 5.5): E1 with |x - r| <= a_j + 5.5, |r| <= R_j + 5.5; a rescale happens only when the
        reference is beaten, each time by a jump > 5.5, so at most (a_j + 5.5) / 5.5 times, E2 with differences that
        telescope to <= a_j + 5.5; the lane pair shares the reference (plain addition); the finalize kernel is an E2:
            rel_j = 8 (a_j + 5.5) + 3 (a_j + 5.5) / 5.5 + R_j + 5.5 + 5 + depth_j
    FORM_QFWD (qfwd2 / qfwd3; FIXED reference per (slice, row): the maximum of the slice's first 32-item tile plus
        QF_REF_MARGIN, 0 when that tile is all -inf; known from the reference itself): one E1 with the actual
        x_j = |s_j - ref|, no rescale; the finalize kernel is an E2 against ms = the largest reference of the row:
            rel_j = 2 x_j + |ref| + 2 + 3 |ref - ms| + 3 + depth_j
  |log L| = |lse - ms|: ms = M (FORM_LSE), within [M, M + 5.5] (FORM_FUSED: the larger of |lse - M| and
  |lse - M - 5.5| is used), the largest reference (FORM_QFWD).  v_exp_f32 may flush results below 2^-126: at most N 2^-126 e^8 of L, added as 1e-30.
No measured slack anywhere: a ratio err / bound above 1 is a finding."""
from __future__ import annotations

from functools import lru_cache

import numpy as np

U32 = 2.0 ** -24
C_MFMA = 2.0
QS_REF_MARGIN = 5.5
QF_REF_MARGIN = 8.0
LOG2E32 = np.float32(1.4426950408889634)
FORM_LSE, FORM_FUSED, FORM_QFWD = "lse", "fused", "qfwd"
ROW_BLOCK = 256


def _f64(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


# ---- ports of the host-side split functions ------------------------------------------------------------------------------
def qs_choose_split(n_str, n_res, spw, unit_rows, target):
    """qhead.hip qs_choose_split -> (nsplit, split_rows, rblks)"""
    rblks = (n_res + 128 * spw - 1) // (128 * spw)
    units = (n_str + unit_rows - 1) // unit_rows
    want = (target + rblks - 1) // rblks
    max_split = max(1, units // 2)
    want = min(want, max_split)
    if want > 8:
        want = (want + 7) // 8 * 8
    want = max(1, min(want, max_split))
    upb = (units + want - 1) // want
    split_rows = upb * unit_rows
    return (n_str + split_rows - 1) // split_rows, split_rows, rblks


def fwd_split(rows, n_items):
    """cqlrec_qhead_fwd, skeleton forms (QM_LSE, QM_ARGMAX): QS_SPW_FWD = 2, QS_TI = 64, QS_TARGET_BLOCKS = 768"""
    return qs_choose_split(n_items, rows, 2, 64, 768)[:2]


def qargmax2_supported(d, n_items):
    return d in (128, 256) and n_items * 2 * d < 2 ** 31


def qargmax2_split(rows, n_items):
    """qhead_argmax2.hip cql_qargmax2_split -> (nsplit, split_rows)"""
    rblks = (rows + 255) // 256
    units = (n_items + 63) // 64
    want = min((256 + rblks - 1) // rblks, units // 8)
    if want > 8:
        want = want // 8 * 8
    want = max(want, 1)
    split_rows = (units + want - 1) // want * 64
    return (n_items + split_rows - 1) // split_rows, split_rows


def fused_form(d, n_items):
    """which kernel cqlrec_qhead_fwd_lse_dh launches first: "qfwd2" (d = 128), "qfwd3" (d = 256), "generic" (QM_LSE_DH)"""
    if d == 128 and n_items * 256 < 2 ** 31:
        return "qfwd2"
    if d == 256 and n_items * 512 < 2 ** 31:
        return "qfwd3"
    return "generic"


def fused_split(rows, n_items, d):
    """fused_ws' choice: QS_SPW_BWD = 1, QS_TARGET_BLOCKS_BWD = 512, halved where qfwd3 runs"""
    return qs_choose_split(n_items, rows, 1, 64, 256 if fused_form(d, n_items) == "qfwd3" else 512)[:2]


def argmax_geometry(d, rows, n_items, step=False):
    """(form, stage length, nsplit, split_rows) of the ARGMAX pass: through cqlrec_qhead_fwd, or (step) as the training
    step launches it -- the skeleton at d = 128 even where qargmax2 is supported"""
    if d != 64 and qargmax2_supported(d, n_items) and not (step and d == 128):
        ns, sr = qargmax2_split(rows, n_items)
        return "qargmax2", (64 if d == 128 else 32), ns, sr
    ns, sr = fwd_split(rows, n_items)
    return "skeleton", (32 if d == 256 else 64), ns, sr


# ---- exact scores -------------------------------------------------------------------------------------------------------------
def scores64(H, E, b, block=ROW_BLOCK):
    """yields (lo, hi, S, e): S = H E^T + b in float64 for rows lo..hi-1, e the per-item score bound (0 where S = -inf)"""
    H64, E64, b64 = _f64(H), _f64(E), _f64(b)
    d = H64.shape[1]
    Ea, ba = np.abs(E64).T.copy(), np.where(np.isfinite(b64), np.abs(b64), 0.0)
    Et = E64.T.copy()
    for lo in range(0, H64.shape[0], block):
        hi = min(H64.shape[0], lo + block)
        S = H64[lo:hi] @ Et
        S += b64
        e = np.abs(H64[lo:hi]) @ Ea
        e += ba
        e *= (d + 1) * C_MFMA * U32
        e[~np.isfinite(S)] = 0.0
        yield lo, hi, S, e


def mfma_row(reg, half):
    """common.h mfma_row: the tile row of accumulator register `reg` in lane half `half`"""
    return (reg & 3) + 8 * (reg >> 2) + 4 * half


def lane_half_of_row(row):
    return next(h for h in (0, 1) for reg in range(16) if mfma_row(reg, h) == row % 32)


class Form:
    """one kernel form's slice geometry for the lse bound"""

    def __init__(self, kind, nsplit, split_rows, n_items):
        assert kind in (FORM_LSE, FORM_FUSED, FORM_QFWD)
        self.kind, self.nsplit, self.split_rows, self.n_items = kind, int(nsplit), int(split_rows), int(n_items)
        j = np.arange(n_items)
        self.slice_of = j // self.split_rows
        in_slice = j - self.slice_of * self.split_rows
        slice_len = np.minimum(self.split_rows, n_items - self.slice_of * self.split_rows)
        self.tiles_after = (slice_len + 31) // 32 - 1 - in_slice // 32            # T_j
        self.depth = 17.0 + self.tiles_after + 1.0 + (self.nsplit - self.slice_of)


def lse_forms(B, Nn, d):
    """name -> Form of every lse form the two ABI entries can reach at this shape: "fwd_lse" (cqlrec_qhead_fwd, QM_LSE),
    the first kernel of cqlrec_qhead_fwd_lse_dh ("qfwd2" / "qfwd3", or "fused_generic" at d = 64) and "fused_generic" as
    the guarded fall-back behind qfwd2 / qfwd3 (same slices)"""
    ns, sr = fwd_split(B, Nn)
    fs, fr = fused_split(B, Nn, d)
    forms = {"fwd_lse": Form(FORM_LSE, ns, sr, Nn), "fused_generic": Form(FORM_FUSED, fs, fr, Nn)}
    if fused_form(d, Nn) != "generic":
        forms[fused_form(d, Nn)] = Form(FORM_QFWD, fs, fr, Nn)
    return forms


def _lse_rows(S):
    M = S.max(1)
    Ms = np.where(np.isfinite(M), M, 0.0)
    with np.errstate(divide="ignore"):
        P = np.exp(S - Ms[:, None])
        L = P.sum(1)
        lse = Ms + np.log(L)
    with np.errstate(invalid="ignore", divide="ignore"):
        P /= L[:, None]
    P[~np.isfinite(P)] = 0.0
    return M, lse, P


def _bound_rows(form, S, e, M, lse, P):
    """bound_lse of the rows of one block for one form; (bound, per-(row, slice) log of the partial sum or None)"""
    fin = np.isfinite(S)
    Sf = np.where(fin, S, 0.0)
    Mf = np.where(np.isfinite(M), M, 0.0)[:, None]
    a = np.where(fin, Mf - Sf, 0.0)
    R = np.where(fin, np.maximum(np.abs(Mf), np.abs(Sf)), 0.0)
    T, depth = form.tiles_after[None, :], form.depth[None, :]
    part_log = None
    if form.kind == FORM_LSE:
        rel = 10.0 * a + (1.0 + T) * R + 3.0 * T + 8.0 + depth
        logL = np.abs(lse - Mf[:, 0])
    elif form.kind == FORM_FUSED:
        am = a + QS_REF_MARGIN
        rel = 8.0 * am + 3.0 * am / QS_REF_MARGIN + R + QS_REF_MARGIN + 5.0 + depth
        logL = np.maximum(np.abs(lse - Mf[:, 0]), np.abs(lse - Mf[:, 0] - QS_REF_MARGIN))
    else:
        ref = np.empty((S.shape[0], form.nsplit))
        part_log = np.empty_like(ref)
        for k in range(form.nsplit):
            lo = k * form.split_rows
            m1 = S[:, lo: lo + 32].max(1)
            ref[:, k] = np.where(np.isfinite(m1), m1 + QF_REF_MARGIN, 0.0)
            sl = S[:, lo: lo + form.split_rows] - ref[:, k: k + 1]
            mk = sl.max(1)
            mks = np.where(np.isfinite(mk), mk, 0.0)
            with np.errstate(divide="ignore"):
                part_log[:, k] = mks + np.log(np.exp(sl - mks[:, None]).sum(1))
        ms = ref.max(1)
        rj = ref[:, form.slice_of]
        rel = 2.0 * np.where(fin, np.abs(Sf - rj), 0.0) + np.abs(rj) + 2.0 + 3.0 * np.abs(rj - ms[:, None]) + 3.0 + depth
        logL = np.abs(lse - ms)
    x = U32 * (P * rel).sum(1)
    emax = e.max(1)
    bound = np.exp(2.0 * emax) * (P * e).sum(1) + x + x * x + 6.0 * U32 * logL + U32 * np.abs(lse) + 1e-30
    bound = np.where(np.isfinite(lse), bound, 0.0)                 # a row with nothing finite: lse = -inf exactly
    return bound, part_log


class LseReference:
    """lse64, the row maximum, argmax_first, the smallest probability of each row and, per requested form, bound_lse and
    (FORM_QFWD) whether a partial sum overflows fp32 -- the condition of the guarded fall-back"""

    def __init__(self, H, E, b, forms):
        rows = np.asarray(H).shape[0]
        self.lse, self.M = np.empty(rows), np.empty(rows)
        self.argmax = np.empty(rows, np.int64)
        self.pmin = np.empty(rows)
        self.bound = {name: np.empty(rows) for name in forms}
        self.overflow = {name: False for name in forms}
        self.forms = forms
        fin_b = np.isfinite(np.asarray(b, dtype=np.float64))
        for lo, hi, S, e in scores64(H, E, b):
            M, lse, P = _lse_rows(S)
            self.lse[lo:hi], self.M[lo:hi] = lse, M
            self.argmax[lo:hi] = S.argmax(1)
            self.pmin[lo:hi] = P[:, fin_b].min(1) if fin_b.any() else 0.0
            for name, form in forms.items():
                bd, part_log = _bound_rows(form, S, e, M, lse, P)
                self.bound[name][lo:hi] = bd
                if part_log is not None:
                    big = part_log[np.isfinite(part_log)]
                    # fp32 overflows at ln(3.4e38) = 88.7; the kernel's test is `!(sum < 3e38)`
                    assert not ((big > 86.0) & (big < 91.0)).any(), "partial sum too close to the fp32 limit to predict"
                    self.overflow[name] |= bool((big >= 91.0).any())


def check_lse(got, ref: LseReference, name, rows=None):
    """every row: |got - lse64| <= bound_lse[name] (rows with lse64 = -inf: got must be -inf).  Returns the worst
    err / bound; raises AssertionError naming the worst rows."""
    got = np.asarray(got, dtype=np.float64)
    lse, bound = ref.lse, ref.bound[name]
    if rows is not None:
        lse, bound = lse[rows], bound[rows]
    assert got.shape == lse.shape
    dead = np.isneginf(lse)
    ok_dead = np.isneginf(got[dead]).all()
    with np.errstate(invalid="ignore"):
        err = np.where(dead, 0.0, np.abs(got - lse))
        ratio = np.where(err == 0, 0.0, err / bound)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    bad = np.nonzero(~(err <= bound))[0]
    if bad.size or not ok_dead:
        worst = bad[np.argsort(-ratio[bad])][:4]
        raise AssertionError(f"lse rows off ({name}): {bad.size} of {got.size} over the bound" +
                             ("" if ok_dead else "; a row with nothing finite is not -inf") + "; worst: " +
                             ", ".join(f"row {int(r)}: got {got[r]!r} ref {lse[r]!r} err/bound {ratio[r]:.3g}" for r in worst))
    return float(ratio.max(initial=0.0))


def check_argmax(H, E, b, imax, vmax=None):
    """The derived margin rule, per row: the chosen item is admissible (finite score), its exact score is
    >= max_j s_j - (e_got + e_argmax), and vmax (where the caller has it) is within e_got of it.  Returns the worst
    |vmax - s_got| / e_got."""
    imax = np.asarray(imax).astype(np.int64)
    have_v = vmax is not None
    vmax = np.asarray(vmax, dtype=np.float64) if have_v else np.zeros(imax.shape)
    n_items = np.asarray(E).shape[0]
    fails, worst = [], 0.0
    for lo, hi, S, e in scores64(H, E, b):
        r = np.arange(hi - lo)
        g = imax[lo:hi]
        if ((g < 0) | (g >= n_items)).any():
            fails.append(f"rows {lo}..{hi}: index out of range")
            continue
        am = S.argmax(1)
        s_got, e_got = S[r, g], e[r, g]
        with np.errstate(invalid="ignore"):
            bad = ~(s_got >= S[r, am] - (e_got + e[r, am])) | ~np.isfinite(s_got)
            verr = np.abs(vmax[lo:hi] - s_got) if have_v else np.zeros(hi - lo)
            badv = ~(verr <= e_got)
            ratio = np.where(verr == 0, 0.0, verr / np.maximum(e_got, 1e-300))
        worst = max(worst, float(np.nan_to_num(ratio, nan=np.inf).max(initial=0.0)))
        for i in np.nonzero(bad)[0][:3]:
            fails.append(f"row {lo + i}: item {g[i]} scores {s_got[i]!r}, the maximum {S[i, am[i]]!r} at {am[i]}")
        for i in np.nonzero(badv)[0][:3]:
            fails.append(f"row {lo + i}: vmax {vmax[lo + i]!r}, exact score of item {g[i]} {s_got[i]!r}, e {e_got[i]:.3g}")
    assert not fails, "arg-max rows off: " + "; ".join(fails[:8])
    return worst


def exact_argmax(H, E, b):
    """(argmax_first, maximum as float32) -- for dyadic data, where every score is exact in fp32"""
    idx = np.empty(np.asarray(H).shape[0], np.int64)
    val = np.empty(idx.shape, np.float32)
    for lo, hi, S, _ in scores64(H, E, b):
        idx[lo:hi] = S.argmax(1)
        val[lo:hi] = S.max(1).astype(np.float32)
        assert np.array_equal(val[lo:hi].astype(np.float64), S.max(1)), "scores are not exact in fp32: not a dyadic case"
    return idx, val


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
FLAT_AMP, BIAS_AMP = 0.002, 0.005


def bf16_round(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return (r & 0xFFFFFFFF).astype(np.uint32).view(np.float32).reshape(x.shape)


@lru_cache(maxsize=4)
def lse_inputs(B, Nn, d, bias):
    """bf16 states mixing FLAT rows (amplitude FLAT_AMP: every item carries about 1 / N of the sum, so one dropped item
    shows) with peaked ones (0.5, 3, 8), bf16 item table, a small fp32 bias (BIAS_AMP: the bias is the first addend of the
    MFMA chain and its magnitude enters e_j d + 1 times); "ramp": + 0.02 per item id, a running reference keeps being
    beaten; "+200": a step of 200 nats behind the first 40 items, a reference fixed from the first tile overflows.
    Returns (H, E, b, flat) with flat the mask of the flat rows (row 0 always is)."""
    rng = np.random.default_rng(B * 7 + Nn * 3 + d)
    amp = rng.choice([FLAT_AMP, 0.5, 3.0, 8.0], size=B).astype(np.float32)
    amp[0] = FLAT_AMP
    H = bf16_round(rng.standard_normal((B, d)).astype(np.float32) * amp[:, None])
    E = bf16_round((rng.standard_normal((Nn, d)) / np.sqrt(d)).astype(np.float32))
    b = (rng.standard_normal(Nn) * BIAS_AMP).astype(np.float32)
    if bias == "ramp":
        b = (b + 0.02 * np.arange(Nn, dtype=np.float32)).astype(np.float32)
    elif bias == "+200":
        b[40:] += np.float32(200.0)
    else:
        assert bias == "none"
    return H, E, b, amp == np.float32(FLAT_AMP)


def dyadic_inputs(rows, Nn, d, seed):
    """multiples of 1/8 in [-1, 1] (bias: [-2, 2]): every score is a multiple of 1/64 below 2^9, exact in fp32 in any order"""
    rng = np.random.default_rng(seed)
    H = (rng.integers(-8, 9, (rows, d)) / 8.0).astype(np.float32)
    E = (rng.integers(-8, 9, (Nn, d)) / 8.0).astype(np.float32)
    b = (rng.integers(-16, 17, Nn) / 8.0).astype(np.float32)
    return H, E, b


TIE_PATTERNS = ("from_f", "pair", "later_wins")


def tie_layout(E, b, pattern, f, g):
    """Copies of dyadic (E, b) with a prescribed maximum, the same for every state: the marked items get item f's row and a
    bias of 2 d + 4 (their score beats every other item's, |h . e| <= d, |b| <= 2, by more than 2).
      from_f      all items >= f share the maximum                       -> f
      pair        exactly f < g share it                                 -> f
      later_wins  g beats f by one dyadic step (1/8)                     -> g   (guards against "the first tile always wins")
    Returns (E, b, expected arg-max)."""
    E, b = E.copy(), b.copy()
    Nn, d = E.shape
    top = np.float32(2 * d + 4)
    assert 0 <= f < Nn and (pattern == "from_f" or f < g < Nn)
    if pattern == "from_f":
        E[f:], b[f:] = E[f], top
        return E, b, f
    E[g] = E[f]
    b[f] = top
    b[g] = top if pattern == "pair" else top + np.float32(0.125)
    return E, b, (f if pattern == "pair" else g)


def tie_positions(stage, tile, split_rows, n_items, parity=False):
    """The (f, g) that matter for a kernel geometry (stage length, tile length, slice length, N), g < N, f < g:
    same lane (0, 1); the two lane halves of one tile (rows 3 and 4: mfma_row puts rows 0..3 in half 0, 4..7 in half 1);
    adjacent tiles; a stage boundary; (parity: one tile per stage, register sets alternating) the boundaries in front of
    even stages 2 and 4; the first slice boundary; the first item against the last; the last two items."""
    assert lane_half_of_row(0) == lane_half_of_row(1) and lane_half_of_row(3) != lane_half_of_row(4)
    cand = [(0, 1), (3, 4), (tile - 1, tile), (stage - 1, stage), (split_rows - 1, split_rows), (0, n_items - 1),
            (n_items - 2, n_items - 1)]
    if parity:
        cand += [(stage * 2 * k - 1, stage * 2 * k) for k in (1, 2)]
        cand += [(stage * 3 - 1, stage * 3)]                     # ... and in front of an odd one
    out = []
    for f, g in cand:
        if 0 <= f < g < n_items and (f, g) not in out:
            out.append((f, g))
    return out


# ---- fp32 port of the lse pipeline (for the CPU self-test) ------------------------------------------------------------------------
def lse_emulate(H, E, b, form, order, mutate=None):
    """The lse of every row as the kernels form it, in fp32: scores in fp32 (order "sgemm": BLAS; "chain16": 16-term
    blocks chained in k order, bias first, as the MFMA chain; "reverse": k descending, bias last), per slice a
    (reference, sum of exp2(fma(s, log2e, -ref log2e))) partial -- reference = slice maximum (+ QS_REF_MARGIN, FORM_FUSED)
    or first-tile maximum + QF_REF_MARGIN (FORM_QFWD) -- summed in fp32 in the same order family, then the merge of
    qhead_finalize_lse_kernel.  mutate(part_ref, part_sum) may alter the partials in place."""
    H32, E32, b32 = (np.asarray(x, dtype=np.float32) for x in (H, E, b))
    d = H32.shape[1]
    if order == "sgemm":
        S = (H32 @ E32.T + b32).astype(np.float32)
    else:
        ks = list(range(0, d, 16))
        S = np.broadcast_to(b32, (H32.shape[0], E32.shape[0])).astype(np.float32) if order == "chain16" else \
            np.zeros((H32.shape[0], E32.shape[0]), np.float32)
        for k in (ks if order == "chain16" else ks[::-1]):
            S = (S + H32[:, k:k + 16] @ E32[:, k:k + 16].T).astype(np.float32)
        if order == "reverse":
            S = (S + b32).astype(np.float32)
    pr = np.empty((form.nsplit, S.shape[0]), np.float32)
    ps = np.empty_like(pr)
    for k in range(form.nsplit):
        sl = S[:, k * form.split_rows: (k + 1) * form.split_rows]
        if form.kind == FORM_QFWD:
            m = sl[:, :32].max(1)
            ref = np.where(np.isfinite(m), m + np.float32(QF_REF_MARGIN), np.float32(0)).astype(np.float32)
        else:
            m = sl.max(1)
            ref = (m + np.float32(QS_REF_MARGIN if form.kind == FORM_FUSED else 0.0)).astype(np.float32)
            ref = np.where(np.isfinite(m), ref, np.float32(-np.inf) if form.kind == FORM_FUSED else np.float32(0)).astype(np.float32)
        rz = np.where(np.isfinite(ref), ref, np.float32(0)).astype(np.float32)
        off = (-rz * LOG2E32).astype(np.float32)
        with np.errstate(over="ignore"):
            P = np.exp2((sl.astype(np.float64) * float(LOG2E32) + off[:, None]).astype(np.float32)).astype(np.float32)
        if order == "sgemm":
            s = P.sum(1, dtype=np.float32)
        else:
            cols = range(P.shape[1]) if order == "chain16" else range(P.shape[1] - 1, -1, -1)
            s = np.zeros(P.shape[0], np.float32)
            for c in cols:
                s = (s + P[:, c]).astype(np.float32)
        pr[k], ps[k] = (ref if form.kind != FORM_LSE else np.where(np.isfinite(m), m, np.float32(-np.inf))), s
    if mutate is not None:
        mutate(pr, ps)
    return finalize_lse(pr, ps)


def finalize_lse(pm, pl):
    """qhead_finalize_lse_kernel in fp32: partials [nsplit, rows] -> (lse, nlse2)"""
    M = pm.max(0)
    ms = np.where(np.isneginf(M), np.float32(0), M).astype(np.float32)
    L = np.zeros(pm.shape[1], np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for k in range(pm.shape[0]):
            w = np.exp2(((pm[k] - ms).astype(np.float32) * LOG2E32).astype(np.float32)).astype(np.float32)
            L = (L + (pl[k] * w).astype(np.float32)).astype(np.float32)
        v = (ms + np.log(L.astype(np.float64)).astype(np.float32)).astype(np.float32)
    return v, (-v * LOG2E32).astype(np.float32)
